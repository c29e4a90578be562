/*
 * pulsarutils_hip.h - C-ABI of the MI355X (gfx950) dedispersion + cleaning library
 * (libpulsarutils_hip.so).  Plain pointers and sizes only; no torch types.
 *
 * The reference (matteobachetti/radio-pulsar-utils, package ``pulsarutils``) is pure
 * Python + numba; it has no FFI of its own.  Each entry point below replaces one
 * reference function (cited file:line, paths relative to the reference root); the
 * Python host layer (radio-pulsar-utils_amd/pulsarutils) binds them with ctypes
 * exactly as INTEGRATION.md shows.
 *
 * Conventions
 *  - Device pointers are owned by the caller (e.g. torch tensors).  Host pointers
 *    are marked "host".  Row-major 2-D arrays carry a leading dimension ``ld``
 *    (elements).
 *  - Calls are asynchronous on ``stream`` (a hipStream_t passed as void*; NULL = the
 *    null stream) and never throw - except pu_plan_search / pu_plan_finalize, which
 *    synchronise ``stream`` once to settle their certification step (see
 *    pu_plan_finalize) and return final outputs.  They return PU_OK (0) or a negative PU_E* code;
 *    pu_last_error() returns a thread-local message for the last failure.
 *  - The caller selects the device (hipSetDevice) before calling.
 */
#ifndef PULSARUTILS_HIP_H
#define PULSARUTILS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* element types */
#define PU_U8 0
#define PU_F32 1
#define PU_F64 2
#define PU_I64 3 /* rebin/roll helpers only */

/* accumulation type of the dedispersion sum */
#define PU_ACC_NATIVE 0 /* u8 -> f32 (exact), f32 -> f32, f64 -> f64 */
#define PU_ACC_F32 1
#define PU_ACC_F64 2 /* float64 accumulator in channel order: bit-exact vs the reference */

/* status codes */
#define PU_OK 0
#define PU_EINVAL (-1)
#define PU_EHIP (-2)
#define PU_ENOMEM (-3)
#define PU_EUNSUPPORTED (-4)

const char *pu_version(void);
const char *pu_last_error(void);

/* ------------------------------------------------------------------ planner (host) */

/* Replaces dedispersion_shifts (pulsarutils/dedispersion.py:125-139) for ``ndm``
 * trials at once.  float64 with CPython scalar semantics (libm pow, float floor
 * division, rint).  host: dms[ndm], out[ndm][nchan]. */
int pu_shift_table(int64_t nchan, const double *dms, int64_t ndm, double start_freq,
                   double bandwidth, double sample_time, int64_t *out);

/* ------------------------------------------------------------------ dedispersion */

typedef struct pu_plan pu_plan;

/* Build a dedispersion plan for ``ndm`` trials over an (nchan, nsamples) filterbank
 * of element type ``dtype``.  host: shifts[ndm][nchan] = the reference's per-channel
 * integer delays (dedispersion_shifts output, any sign).  Tiles DM trials x time,
 * derives per-tile LDS halos and uploads the metadata to the current device.
 * Replaces the per-trial shift computation + normalize_shifts of
 * _dedispersion_search (dedispersion.py:183-184, 97, 101-122). */
int pu_plan_create(pu_plan **plan, int dtype, int acc, int64_t nchan, int64_t nsamples,
                   const int64_t *shifts, int64_t ndm);
/* Same, choosing the float32-accumulation strategy: ``group`` = channels summed into
 * one exact partial-sum row per distinct relative-shift vector:
 * 0 = default (the cheapest of the wide / tall shapes with G = 4 and 8 by the planner's
 * cost model, falling back to smaller groups / channel mode when the trial grid does not
 * suit them), 1 = channel mode, 2/4/8.  Float64 accumulation always runs channel mode
 * (the reference's channel order).  = pu_plan_create_ex with opts {group, -1, 0, -1, -1}. */
int pu_plan_create_grouped(pu_plan **plan, int dtype, int acc, int64_t nchan, int64_t nsamples,
                           const int64_t *shifts, int64_t ndm, int group);

/* Explicit planner options (the production library reads no environment: every
 * strategy choice is an argument here or a default).  -1 / 0 = automatic. */
typedef struct pu_plan_opts {
    int32_t group;          /* 0 auto, 1 channel mode, 2 / 4 / 8 */
    int32_t shape;          /* subband workgroup shape: -1 auto, 0 wide, 1 pair, 2 tall */
    int32_t lds_budget_kb;  /* 0: default (160 KiB subband, 64 KiB channel mode) */
    int32_t u8_dma;         /* -1 auto (8-bit rows by LDS-DMA when n % 4 == 0), 0 global-memory build */
    int32_t dt_major;       /* -1 auto item order, 0 time-tile major, 1 DM-tile major */
    int32_t slot16;         /* 16-bit integer slots for 8-bit rows by LDS-DMA in 256-sample
                             * time tiles: -1 auto (= 1), 0 never (float32 slots), 1 every
                             * group size (round 6: -1 meant groups of <= 4 channels) */
    int32_t reserved[2];    /* zero */
} pu_plan_opts;
int pu_plan_create_ex(pu_plan **plan, int dtype, int acc, int64_t nchan, int64_t nsamples,
                      const int64_t *shifts, int64_t ndm, const pu_plan_opts *opts);
void pu_plan_destroy(pu_plan *plan);

/* What pu_plan_create_ex would build for the same arguments, without building it: the same
 * validation and the same planner run on the host alone (no device is touched, none is
 * needed).  Fills up to ``ninfo`` fields of ``info`` in pu_plan_info's layout (the cert_*
 * fields 0) and, if ``tables_digest`` is not NULL, a 64-bit digest of the tables the plan
 * would upload, padding included: FNV-1a over each table's name, element count (uint64)
 * and bytes, the tables taken in the order of their names (base, count, first, rec, rec8,
 * recs, rowlen, slots, stages, tile_stages, tiles; a table the plan's mode does not use has
 * count 0).  For tests of the planner (tests/test_plan_tables.py pins both against recorded
 * values) and for developing planner changes away from a GPU.  No reference counterpart
 * (the reference computes its shifts per trial, dedispersion.py:183-184). */
int pu_plan_describe(int dtype, int acc, int64_t nchan, int64_t nsamples, const int64_t *shifts,
                     int64_t ndm, const pu_plan_opts *opts, int64_t *info, int ninfo,
                     uint64_t *tables_digest);

/* Device scratch bytes pu_plan_search needs (per-tile partial statistics). */
size_t pu_plan_workspace_bytes(const pu_plan *plan);

/* Replaces _dedispersion_search (dedispersion.py:174-202): for every trial the
 * circular shift-and-sum over channels, mean subtraction, and the S/N of the
 * 1/2/4/8-sample rebinned series; outputs max, std, best snr, best rebin (device,
 * [ndm] each).  data: device (nchan rows of ld elements). */
int pu_plan_search(pu_plan *plan, const void *data, int64_t ld, double *max_out,
                   double *std_out, double *snr_out, int32_t *rebin_out, void *workspace,
                   size_t workspace_bytes, void *stream);

/* pu_plan_search split in two, for pipelining (multi-GPU: the search of early time
 * chunks overlaps the broadcast of later ones).  search_tiles runs the
 * shift-and-sum + per-tile statistics of time tiles [tt_begin, tt_end) only (time
 * tile = pu_plan_info "time_tile" samples; a tile reads its window plus the shift
 * halo, modulo nsamples); once every tile has run, finalize combines the per-tile
 * records into the per-trial outputs exactly as pu_plan_search does. */
int pu_plan_search_tiles(pu_plan *plan, const void *data, int64_t ld, int64_t tt_begin,
                         int64_t tt_end, void *workspace, size_t workspace_bytes, void *stream);
int pu_plan_finalize(pu_plan *plan, const void *data, int64_t ld, double *max_out,
                     double *std_out, double *snr_out, int32_t *rebin_out, void *workspace,
                     size_t workspace_bytes, void *stream);

/* pu_plan_finalize of trials [trial_begin, trial_end) only (time-tile sharding across
 * GPUs, DESIGN.md §5: each rank searches a range of time tiles for every trial, the
 * per-tile records of each trial are moved to the rank that owns the trial, and the owner
 * finalizes its trials).  The records are the workspace's first bytes, trial-major:
 * record (trial d, time tile t) = rec_stride elements of rec_elem_bytes (float32 or
 * float64) at element (d ntt + t) rec_stride (pu_plan_info "rec_elem_bytes",
 * "rec_stride"); only the range's records are read.  Outputs are indexed by plan trial
 * (arrays of ndm; only [trial_begin, trial_end) written).  Certification as in
 * pu_plan_finalize (flagged trials recomputed exactly from data, which must then hold the
 * whole filterbank).  The replaced reference code is the same (dedispersion.py:174-202). */
int pu_plan_finalize_range(pu_plan *plan, const void *data, int64_t ld, int64_t trial_begin,
                           int64_t trial_end, double *max_out, double *std_out, double *snr_out,
                           int32_t *rebin_out, void *workspace, size_t workspace_bytes, void *stream);

/* The finalize of trials [trial_begin, trial_end) without the exact recomputation, for
 * time-tile sharding where each rank holds only its time slice of the filterbank
 * (DESIGN.md §5): the fast statistics are written (outputs indexed by plan trial) and the
 * trials certification would recompute are returned instead - counts[0] = how many,
 * counts[1] = of which with a non-finite partial; the first min(count, cap) plan trial
 * indices into flagged (host, ascending).  Synchronises stream.  The caller settles them
 * (pulsarutils.parallel: a non-finite input anywhere -> the NaN rule for every trial;
 * otherwise each rank's slice of pu_plan_exact_series, gathered, + pu_series_stats). */
int pu_plan_finalize_range_flagged(pu_plan *plan, int64_t trial_begin, int64_t trial_end,
                                   double *max_out, double *std_out, double *snr_out, int32_t *rebin_out,
                                   void *workspace, size_t workspace_bytes, int32_t *flagged, int64_t cap,
                                   int64_t *counts, void *stream);

/* The reference's float64 dedispersed series (channel order, dedispersion.py:86-98, bit
 * for bit) of m plan trials (host indices) at samples [t_begin, t_end) into out (device,
 * m x (t_end - t_begin) contiguous).  Sample t reads column (t + shift) mod nsamples of each
 * channel: a time-split rank computes its own samples from the columns it holds.
 * Synchronises. */
int pu_plan_exact_series(pu_plan *plan, const void *data, int64_t ld, const int32_t *trials, int64_t m,
                         int64_t t_begin, int64_t t_end, double *out, void *stream);

/* *flag (device int32) = 1 if any of the nrows x ncols float32 / float64 elements (row
 * stride ld) is NaN or +-inf, else 0 (always 0 for uint8, and for nrows == 0 or ncols == 0,
 * when data may be NULL).  Asynchronous on stream. */
int pu_nonfinite_any(const void *data, int dtype, int64_t nrows, int64_t ncols, int64_t ld, int32_t *flag,
                     void *stream);

/* Certification (pu_plan_search and pu_plan_finalize).  The fast
 * path's per-trial statistics are summed in another order than numpy's; a trial whose
 * result that order could change - a zero or rounding-level std (constant input), a
 * non-finite value, or (float64 accumulation, and uint8 input with exact float32 sums)
 * two windows' S/N within the rounding bound of each other - is recomputed exactly:
 * its series by float64 channel-order dedispersion (bit-identical to the reference's
 * dedisperse) and its statistics by pu_series_stats.  An input holding NaN or +-inf
 * gives every trial the reference's result max = std = NaN, snr = 0, rebin = 0.
 * Both calls therefore synchronise ``stream`` once before returning (the outputs are
 * final when they return).  pu_plan_info reports the trials of the last call that
 * were recomputed ("cert_rechecked") and whether the NaN rule applied ("cert_nan"). */

/* The reference's statistics of given float64 dedispersed series, in numpy's exact
 * order (dedispersion.py:186-201, bit-exact): for each row r of series (rows x n,
 * leading dimension ld) max = np.max(s), std = np.std(s) with s = row - np.mean(row),
 * and the best S/N over the 1/2/4/8-sample rebinned s (quick_resample order) with the
 * reference's strict first-best rule from (0, 0).  Outputs go to position index[r]
 * (device int32; NULL = r).  workspace: 256-byte aligned; rows are processed in
 * batches of as many as pu_series_stats_workspace_bytes(batch, n) <= workspace_bytes
 * allows (at least one). */
size_t pu_series_stats_workspace_bytes(int64_t rows, int64_t n);
int pu_series_stats(const double *series, int64_t rows, int64_t n, int64_t ld,
                    const int32_t *index, double *max_out, double *std_out, double *snr_out,
                    int32_t *rebin_out, void *workspace, size_t workspace_bytes, void *stream);

/* Single-pulse events of float64 dedispersed series (this project's definition; the
 * quantities are those of dedispersion.py:186-201, in the same numpy order as
 * pu_series_stats).  For each row d (rows x n, leading dimension ld) and threshold
 * (finite, > 0):
 *   s = d - np.mean(d)
 *   for window w in 1, 2, 4, 8 with nb = n // w >= 1:
 *       reb = quick_resample(s, w), sd = np.std(reb)
 *       sd not finite or not > 0: no events of this window
 *       bin i is above when reb[i] / sd > threshold (one IEEE division; NaN compares false)
 *       an event is a maximal run [start, start + nbins) of consecutive above bins (the
 *       series is linear: no run wraps from nb - 1 to 0); peak = the first bin of the run
 *       where reb is largest; snr = reb[peak] / sd.
 * So a row has an event iff the reference's snr of it exceeds threshold, and its largest
 * event snr then equals that snr bit for bit.  Events are delivered sorted by (input row r,
 * window, start); pu_event.row is index[r] (device int32; NULL = r).  *count (host)
 * receives the total number of events; the first min(*count, cap) are written to events
 * (device; may be NULL when cap == 0: the call then only counts).  workspace: 256-byte
 * aligned device memory; rows are processed in batches of as many as
 * pu_series_events_workspace_bytes(batch, n) <= workspace_bytes allows (at least one) and
 * the result does not depend on the batch size.  Synchronises stream once. */
typedef struct pu_event {
    int32_t row, window;
    int64_t start, nbins, peak;
    double snr;
} pu_event;
size_t pu_series_events_workspace_bytes(int64_t rows, int64_t n);
int pu_series_events(const double *series, int64_t rows, int64_t n, int64_t ld, const int32_t *index,
                     double threshold, pu_event *events, int64_t cap, int64_t *count, void *workspace,
                     size_t workspace_bytes, void *stream);

/* Replaces dedisperse (dedispersion.py:93-98) for every trial of the plan: writes
 * the dedispersed plane plane[trial * ld_plane + t] in the accumulation type
 * (float32 or float64), the show=True plane of dedispersion_search (:214-227). */
int pu_plan_dedisperse(pu_plan *plan, const void *data, int64_t ld, void *plane,
                       int64_t ld_plane, void *stream);

/* The plan's DM tiles in launch order (tile t = trials first[t] .. first[t] + count[t] - 1);
 * writes up to ``n`` of each (either pointer may be NULL) and returns the tile count. */
int pu_plan_dm_tiles(const pu_plan *plan, int32_t *first, int32_t *count, int n);
/* pu_plan_dedisperse restricted to one DM tile ``dt`` of the plan: the tile's trials'
 * rows (dedispersion.py:93-98) at plane rows 0 .. count[dt] - 1, computed by the very
 * kernel instantiation, tables and tiling a full launch of the plan uses (parity tests
 * of a production plan's series at full size without its whole plane). */
int pu_plan_dedisperse_dm_tile(pu_plan *plan, const void *data, int64_t ld, int64_t dt,
                               void *plane, int64_t ld_plane, void *stream);

/* Measurement (bench.py): record a HIP event pair on the launch stream around each
 * of the next ``nslots`` dedispersion-kernel launches of this plan (0 disables). */
int pu_plan_enable_timing(pu_plan *plan, int nslots);
/* Synchronises on the recorded events and writes up to ``n`` kernel durations (ms,
 * launch order).  Returns the number written, or a negative PU_E* code. */
int pu_plan_kernel_times(pu_plan *plan, float *ms, int n);

/* Diagnostics: in the PU_STAMPS build (make stamps -> libpulsarutils_hip_stamps.so) the
 * first call arms per-phase shader-clock stamps of the subband kernel and returns 0;
 * later calls synchronise, write up to ``n`` (<= 16) summed wave-cycle totals {stall on
 * the stage metadata after barrier A, barrier A wait, build, barrier B wait, DMA issue,
 * sum, epilogue, -}, first of the waves that issue no DMA, then of the DMA-issuing
 * waves, and reset them.  Returns 0 in the production build. */
int pu_plan_stamps(pu_plan *plan, int64_t *out, int n);

/* Introspection (tests / DESIGN.md): fills up to ``n`` of
 * {ndm, dm_tiles, time_tiles, trials_per_tile, time_tile, chans_per_step,
 *  row_stride, lds_bytes, acc_is_f64, max_spread, group, slots, stages,
 *  slot_bytes, raw_stride, exec_adds, lds_traffic, cert_rechecked, cert_nan, cert_std,
 *  cert_sign, cert_tie, cert_us, kernel, rec_elem_bytes, rec_stride}: exec_adds and lds_traffic are the adds and LDS bytes (reads,
 *  writes, DMA) one launch executes (subband mode; 0 otherwise); the cert_* fields
 *  describe the last search's certification step (see pu_plan_finalize): trials
 *  recomputed, the NaN rule, and how many trials each check flagged (std not above its
 *  rounding bound, S/N sign, S/N tie) and the host microseconds spent settling them;
 *  kernel: 0 dedisp_kernel (channel order), 1 dedisp_f64_kernel, 2 dedisp_sub_kernel
 *  (float32 slots), 3 dedisp_sub_kernel with 16-bit integer slots (8-bit input);
 *  rec_elem_bytes / rec_stride: the per-(trial, time tile) record layout at the start of
 *  the workspace (pu_plan_finalize_range).  Returns the count written. */
int pu_plan_info(const pu_plan *plan, int64_t *info, int n);

/* ------------------------------------------------------------------ streams */

/* A compute stream on the current device whose CU mask leaves ``reserve`` CUs out
 * (spread over the XCDs), for launching the search while an RCCL collective runs on
 * another stream: the collective's workgroups find those CUs free (the search holds one
 * 160 KiB-LDS workgroup per CU).  No reference counterpart (multi-GPU path, DESIGN.md
 * §5; the reference's parallelism is numba prange, dedispersion.py:181).
 * *stream: hipStream_t as void*, released with pu_stream_destroy. */
int pu_stream_create_cu_masked(int reserve, void **stream);
int pu_stream_destroy(void *stream);

/* ------------------------------------------------------------------ cleaning */

/* Per-row sums in numpy's exact add.reduce order (8192-element blocks, each
 * pairwise-summed), the reductions behind ndarray.mean(1) / np.std(axis=1) in
 * get_noisier_channels (clean.py:60), measure_channel_variability (clean.py:119)
 * and renormalize_data (clean.py:84).
 *   mode 0: sum of x                     (acc: f32 for f32 input, else f64)
 *   mode 1: sum of (x - center[r])^2     (center: device [nrows], acc type)
 *   mode 2: sum of f64(x) * scale[t]     (scale: device [n] f64; acc f64)
 *   mode 3: sum of f64(x)                (acc f64 for every input type)
 *   mode 4: sum of f64(x)^2              (acc f64; get_spectral_stats, stats.py:46-47)
 * out: device [nrows] in the acc type; ``divisor`` > 0 divides each sum in float64
 * and rounds to the acc type (numpy true_divide by the count). */
int pu_row_sums(const void *x, int dtype, int64_t nrows, int64_t n, int64_t ld, int mode,
                const void *center, const double *scale, double divisor, void *out,
                void *workspace, size_t workspace_bytes, void *stream);
size_t pu_row_sums_workspace_bytes(int64_t nrows, int64_t n);

/* One pass for get_noisier_channels + measure_channel_variability (clean.py:60, 119):
 * means[r] = ndarray.mean(1) exactly as pu_row_sums mode 0 with divisor n (f32 for f32
 * input, else f64), and moments[3 r .. 3 r + 2] = (c, sum(x - c), sum((x - c)^2)) in
 * float64, c = x[r, 0], summed in no particular order.  The caller certifies the
 * std-based decisions from the moments (pulsarutils.clean._certified_variability) and
 * runs the exact second pass (pu_row_sums mode 1) only when one is within its rounding
 * bound.  ws: pu_row_moments_workspace_bytes(nrows, n), 8-byte aligned. */
int pu_row_moments(const void *x, int dtype, int64_t nrows, int64_t n, int64_t ld, void *means,
                   double *moments, void *workspace, size_t workspace_bytes, void *stream);
size_t pu_row_moments_workspace_bytes(int64_t nrows, int64_t n);

/* Column means over the rows with skip[r] == 0, sequential in row order
 * (renormalize_data's zero-DM light curve, clean.py:77).  out: device [n] f64. */
int pu_col_means(const void *x, int dtype, int64_t nrows, int64_t n, int64_t ld,
                 const uint8_t *skip, double *out, void *stream);

/* scipy.ndimage.gaussian_filter of a 1-D float64 series, mode 'reflect', in
 * scipy's symmetric correlate1d order (clean.py:79).  weights: device [2r+1]. */
int pu_gaussian_filter1d(const double *x, int64_t n, const double *weights, int64_t radius,
                         double *out, void *stream);

/* factor[t] = numerator / x[t] (clean.py:80). */
int pu_ratio(double numerator, const double *x, int64_t n, double *out, void *stream);

/* np.median of a float64 device series (clean.py:80 ``np.median(lc_smooth)``) into
 * out[0] on the device, bit-exact: radix select of the two middle order statistics,
 * numpy's mean of them; NaN if any element is NaN.  ws: pu_median_workspace_bytes(),
 * 8-byte aligned. */
/* get_noisier_channels' decision (pulsarutils/clean.py:58-67 with stats.py:11-32 ref_mad):
 * mask[i] = spec[i] > medfilt(spec, 7)[i] + 5 * ref_mad(spec), numpy's dtypes and order
 * (spec float32 for float32 input, float64 otherwise; mad_c = statsmodels' MAD constant
 * norm.ppf(3/4)).  One workgroup, 2 <= n <= 4096.  *flag = 1 (mask not written) when spec
 * holds a NaN / inf: the caller decides those on the host. */
int pu_noisy_channels(const void *spec, int dtype, int64_t n, double mad_c, uint8_t *mask, int32_t *flag,
                      void *stream);

/* measure_channel_variability's decision (pulsarutils/clean.py:114-133) certified from
 * the means pass: means[nrows] (dtype PU_F32 / PU_F64: numpy's mean dtype) and
 * moments[nrows][3] = (c, sum(x - c), sum((x - c)^2)) in float64 (pu_row_moments), n
 * samples per row; mef, gam, u: the error factors of clean._certified_variability (the
 * moments' relative error bound, numpy's std summation bound, the unit roundoff).
 * mask[i] = std outside the quartile limits, or bad[i].  One workgroup, nrows <= 4096.
 * *flag = 1 (mask not written, or not certified) for non-finite statistics, too few good
 * channels for the reference's quartile indices, or a channel within its bound of a
 * limit: the caller then computes numpy's std exactly (pu_row_sums mode 1). */
int pu_variability_cert(const void *means, int dtype, const double *moments, int64_t nrows, int64_t n,
                        double mef, double gam, double u, const uint8_t *bad, uint8_t *mask,
                        int32_t *flag, void *stream);

/* get_noisier_channels and then measure_channel_variability(badchans_mask=<that mask>)
 * (pulsarutils/clean.py:58-67, then :114-133) in ONE launch: pu_noisy_channels' decision on
 * spec = means (noisy[nrows], *noisy_flag), then pu_variability_cert's with the noisy mask
 * as bad (var[nrows], *var_flag), same arguments and flag meanings as those two calls
 * (mad_c: pu_noisy_channels'; mef, gam, u: pu_variability_cert's).  One workgroup,
 * 2 <= nrows <= 1024; a non-finite spec sets both flags. */
int pu_channel_masks(const void *means, int dtype, const double *moments, int64_t nrows, int64_t n,
                     double mad_c, double mef, double gam, double u, uint8_t *noisy,
                     int32_t *noisy_flag, uint8_t *var, int32_t *var_flag, void *stream);

size_t pu_median_workspace_bytes(void);
int pu_median(const double *x, int64_t n, double *out, void *ws, size_t ws_bytes, void *stream);

/* factor[t] = numerator[0] / x[t] with the numerator in device memory (clean.py:80). */
int pu_ratio_dev(const double *numerator, const double *x, int64_t n, double *out, void *stream);

/* renormalize_data's light-curve chain (clean.py:77-82 after the zero-DM column means):
 * lc_smooth = gaussian_filter(lc, sigma) (weights: device [2r+1], as pu_gaussian_filter1d),
 * med = np.median(lc_smooth) (as pu_median), factor[t] = med / lc_smooth[t] (as
 * pu_ratio_dev) - those three calls on one stream, with their scratch in one workspace.
 * median_out: device [1] or NULL.  ws: pu_lc_factor_workspace_bytes(n), 256-byte aligned. */
size_t pu_lc_factor_workspace_bytes(int64_t n);
int pu_lc_factor(const double *lc, int64_t n, const double *weights, int64_t radius, double *factor,
                 double *median_out, void *ws, size_t ws_bytes, void *stream);

/* renormalize_data apply pass (clean.py:81-94): out[c][t] = bad[c] ? 0 :
 * (f64(x[c][t]) * factor[t] - spec[c]) / spec[c]; if col_means != NULL it also
 * writes the sequential column mean of ``out`` (the cut_outliers light curve). */
int pu_renorm_apply(const void *x, int dtype, int64_t nchan, int64_t n, int64_t ld,
                    const double *factor, const double *spec, const uint8_t *bad,
                    double *out, int64_t ld_out, double *col_means, void *stream);

/* Opt-in zero-DM subtraction (BASELINE north_star "zero-DM subtraction"; the reference
 * has no counterpart: clean.py:77-82 only DIVIDES by the smoothed zero-DM series, so
 * renormalize_data keeps this off by default).  As pu_renorm_apply, then for every
 * good channel out[c][t] -= S[t] / ngood, S[t] = the in-order sum over channels of the
 * normalised values (bad channels contribute +0.0); bad channels stay 0.  ngood =
 * the number of channels with bad[c] == 0.  col_means (if not NULL) is S[t] / nchan,
 * i.e. the cut_outliers light curve of the data BEFORE the subtraction. */
int pu_renorm_apply_zero_dm(const void *x, int dtype, int64_t nchan, int64_t n, int64_t ld,
                            const double *factor, const double *spec, const uint8_t *bad,
                            int64_t ngood, double *out, int64_t ld_out, double *col_means,
                            void *stream);

/* cut_outliers of renormalize_data (clean.py:93-105) on the device: from the column
 * means lc[n] of the renormalised plane (pu_renorm_apply's col_means), mask[t] =
 * uniform_filter1d(lc, 16)[t] > 5 sd  or  < -3 sd, sd = np.std(uniform_filter1d(lc,
 * 16)[::16]), and out[:, t] = 0 where mask[t].  scipy's running-sum order is not
 * reproducible in parallel: every decision is first made on directly summed windows and
 * CERTIFIED against a rigorous rounding bound of both orders; when a decision is closer
 * to its threshold than the bound (or a value is NaN) the flag word ws[0:4] (uint32) is
 * set and a one-workgroup kernel on the same stream recomputes the mask with scipy's and
 * numpy's own arithmetic (running sum, add.reduce order).  Either way the mask and the
 * zeroed columns are the reference's, with no host round trip (round 4: the caller used
 * to redo the step with scipy).  ws[4:8] (uint32) = number of bad bins.  n >= 64; ws:
 * pu_cut_outliers_workspace_bytes(n), 8-byte aligned.
 * pu_cut_outliers_exact: the exact path only (testing, or callers that want it). */
size_t pu_cut_outliers_workspace_bytes(int64_t n);
int pu_cut_outliers(const double *lc, int64_t n, double *out, int64_t nrows, int64_t ld_out,
                    uint8_t *mask, void *workspace, size_t workspace_bytes, void *stream);
int pu_cut_outliers_exact(const double *lc, int64_t n, double *out, int64_t nrows, int64_t ld_out,
                          uint8_t *mask, void *workspace, size_t workspace_bytes, void *stream);

/* out[:, cols[k]] = 0 for k < ncols (clean.py:105). cols: device int64. */
int pu_zero_columns(double *out, int64_t nrows, int64_t ld_out, const int64_t *cols,
                    int64_t ncols, void *stream);

/* ------------------------------------------------------------------ rebin / roll */

/* quick_resample (dedispersion.py:38-57): out[r][i] = 0 + sum_{j<w} x[r][i*w+j]
 * in float64, i < n/w. */
int pu_rebin_time(const void *x, int dtype, int64_t nrows, int64_t n, int64_t ld,
                  int64_t rebin, double *out, void *stream);

/* quick_chan_rebin (dedispersion.py:15-35): out[g][t] = sum_{j<r} x[g*r+j][t]
 * sequentially; output type: f32->f32, f64->f64, u8->u64, i64->i64. */
int pu_rebin_chan(const void *x, int dtype, int64_t nrows, int64_t n, int64_t ld,
                  int64_t rebin, void *out, void *stream);

/* apply_dm_shifts_to_data (dedispersion.py:254-258): out[c][t] =
 * x[c][(t + shift[c]) mod n] (shift = rint of the reference shift; any sign). */
int pu_roll_rows(const void *x, int dtype, int64_t nrows, int64_t n, int64_t ld,
                 const int64_t *shifts, void *out, void *stream);

/* roll_and_sum (dedispersion.py:60-83), in place on a float64 accumulator:
 * sum[t] += f64(x[(t - roll) mod n]). */
int pu_roll_and_sum(const void *x, int dtype, int64_t n, int64_t roll, double *sum,
                    void *stream);

/* (rows, cols) -> (cols, rows) transpose of 1/2/4/8-byte elements: the time-major ->
 * channel-major reordering sigpyproc's FilReader.readBlock performs on SIGPROC data
 * (clean.py:327, stats.py:45).  dst[c * ld_dst + r] = src[r * ld_src + c]. */
int pu_transpose(const void *src, int elem_bytes, int64_t rows, int64_t cols, int64_t ld_src,
                 void *dst, int64_t ld_dst, void *stream);

/* Unpack + transpose a block of packed SIGPROC samples: src is time-major, one spectrum
 * per row of ld_src BYTES, channel c of a spectrum in bits [c*nbits, (c+1)*nbits) counted
 * from the least-significant bit of byte 0 (sigproc / sigpyproc order: the first channel
 * sits in the low bits).  dst[c * ld_dst + t] =
 *     (src[t * ld_src + (c * nbits) / 8] >> ((c * nbits) % 8)) & ((1 << nbits) - 1)
 * as uint8, channel-major (nchans rows of ld_dst >= nsamps).  nbits 1, 2 or 4;
 * nchans * nbits must be a multiple of 8; ld_src >= nchans * nbits / 8.  src needs no
 * alignment (ld_src may be odd).  Replaces the unpack + transpose of sigpyproc's
 * readBlock (clean.py:327, stats.py:45). */
int pu_unpack_transpose(const void *src, int nbits, int64_t nsamps, int64_t nchans,
                        int64_t ld_src, uint8_t *dst, int64_t ld_dst, void *stream);

/* Quantise + pack + transpose a cleaned block back to SIGPROC sample rows: the inverse of
 * pu_unpack_transpose, and the array step of cleanup_data (clean.py:354-356, a stub in the
 * reference: the requantisation below is this project's definition).  src is channel-major,
 * nchans rows of ld_src ELEMENTS of type dtype (PU_U8 / PU_F32 / PU_F64); dst is time-major,
 * nsamps rows of ld_dst BYTES.  scale, offset: device [nchans] float64, or both NULL for
 * identity (one NULL and one not: PU_EINVAL).
 *     v = (double)src[c * ld_src + t] * scale[c] + offset[c]      (v = x in identity mode)
 * with the multiply and the add rounded separately (no FMA).
 *  nbits 1, 2, 4, 8:  a NaN v is replaced by offset[c] (0 in identity mode: a cleaned sample
 *     of an all-zero channel lands on the mean level), then
 *     q = min(max(rint(v), 0), 2^nbits - 1), rint rounding half to even as np.rint; +-inf
 *     clamp like any other value.  q goes to bits [c*nbits, (c+1)*nbits) of row t counted
 *     from the least-significant bit of byte 0 (at 8 bits the byte is q).  nchans * nbits
 *     must be a multiple of 8; ld_dst >= nchans * nbits / 8; a row's bytes beyond that are
 *     not written.
 *  nbits 32:  row t holds nchans float32 (float)v, round to nearest, no clamp, NaN stays
 *     NaN; ld_dst >= 4 * nchans, dst and ld_dst multiples of 4.
 * src needs the alignment of its element type only and dst none (ld_src and ld_dst may be
 * odd): the access widths follow the pointers and leading dimensions.  PU_EUNSUPPORTED for
 * other nbits / dtypes, PU_EINVAL for bad sizes, PU_OK without a launch for an empty block;
 * all checked before any HIP call. */
int pu_quantize_pack_transpose(const void *src, int dtype, int64_t nchans, int64_t nsamps, int64_t ld_src,
                               const double *scale, const double *offset, int nbits,
                               void *dst, int64_t ld_dst, void *stream);

/* ------------------------------------------------------------------ folding / H-test */

/* Fold a chunk at a pulse period.  No reference counterpart: the reference's PulseInfo
 * (clean.py:27-55) and its dedispersion_search (clean.py:136-180, sample_time = 1 / pulse_freq
 * / nbin) take a folded profile, and nothing in it makes one from a filterbank.
 * x: device, nchan rows of ld elements (PU_U8 / PU_F32 / PU_F64).  Sample t (0 <= t < n) falls
 * in bin b(t), every step one IEEE float64 operation and no fused multiply-add:
 *     p = phase0 + (double)(first_sample + t) * dphase
 *     f = p - floor(p)
 *     b = min((int64)(f * (double)nbin), nbin - 1)
 * (numpy's elementwise phase0 + idx.astype(float64) * dphase gives the same bits, bin edges
 * included).  The call ACCUMULATES: sums[c * ld_sums + b] += the sum of (double)x[c][t] over
 * the t with b(t) = b, counts[b] += their number (device; the caller zeroes both before the
 * first chunk; first_sample = the chunk's position in the file, so the folds of the chunks
 * add up to the fold of the file).  Arithmetic: no floating-point atomics; the order of every
 * sum is fixed by the arguments (segments of 16384 samples from the chunk's start, groups of
 * 64 samples inside them; the per-segment partials are added in segment order, then to
 * sums), so equal calls give equal bits on any device and launch shape.  Exact for PU_U8 and
 * whenever the values and partial sums are integers below 2^53; otherwise each call's
 * addend is within m 2^-53 sum|x| of the exact sum of the bin's m samples.
 * PU_EINVAL: nbin < 1, n < 0, ld < n, ld_sums < nbin, a non-finite phase0 / dphase, |p| >=
 * 2^52 at either end of the chunk, a workspace smaller than pu_fold_workspace_bytes(nchan, n,
 * nbin) or not 8-byte aligned.  PU_EUNSUPPORTED: nbin > 8192 (a channel tile's bins are LDS
 * accumulators; there is no slower path).  PU_OK without a launch for n == 0 or nchan == 0.
 * All checked before any HIP call; asynchronous on stream. */
size_t pu_fold_workspace_bytes(int64_t nchan, int64_t n, int64_t nbin);
int pu_fold(const void *x, int dtype, int64_t nchan, int64_t n, int64_t ld, int64_t first_sample,
            double phase0, double dphase, int64_t nbin, double *sums, int64_t ld_sums,
            int64_t *counts, void *workspace, size_t workspace_bytes, void *stream);

/* The binned Z^2_n and H-test (de Jager et al. 1989) of float64 profiles, in the form of
 * hendrics' / stingray's h_test, which plot_diagnostics calls on every DM row (clean.py:252-253;
 * hendrics itself is no dependency here, so this definition is the project's).  For each row
 * p[0 .. n) of profiles (device, rows x n, leading dimension ld):
 *     P     = sum_j p[j]
 *     C_k   = sum_j p[j] cos(2 pi r / n),  S_k = sum_j p[j] sin(2 pi r / n),  r = (k j) mod n
 *     Z^2_m = (2 / P) sum_{k = 1 .. m} (C_k^2 + S_k^2),   m = 1 .. nmax
 *     H     = max_m (Z^2_m - 4 m + 4),   M = the first m that attains it
 * with r an exact integer, the phases from a table of n sincospi values and the sum over k
 * accumulated sequentially.  h[rows], m[rows] (device); zs (device, may be NULL): Z^2_1 ..
 * Z^2_nmax per row, leading dimension ld_zs.  A row with a non-finite value or with P not > 0
 * gets H = NaN, M = 0 and NaN in zs.  2 <= n <= 8192 and 1 <= nmax <= n - 1 (PU_EINVAL);
 * n > 8192 is PU_EUNSUPPORTED: the H curve of an unfolded chunk (n ~ 1e5, nmax = n / 10) needs
 * an FFT, which this library does not have.  workspace: pu_h_test_workspace_bytes(rows, n,
 * nmax), 16-byte aligned.  All checked before any HIP call; asynchronous on stream. */
size_t pu_h_test_workspace_bytes(int64_t rows, int64_t n, int64_t nmax);
int pu_h_test(const double *profiles, int64_t rows, int64_t n, int64_t ld, int64_t nmax, double *h,
              int32_t *m, double *zs, int64_t ld_zs, void *workspace, size_t workspace_bytes,
              void *stream);

/* Fold series at many trial frequencies: the pulse-frequency search (no reference counterpart:
 * the reference's PulseInfo takes pulse_freq as given).  x: device, rows series of n samples,
 * leading dimension ld (PU_F32 / PU_F64; PU_U8 is PU_EUNSUPPORTED: a dedispersed series is never
 * 8-bit).  phase0, dphase: device [ntrials] float64; phase0 == NULL means 0 for every trial.  For
 * trial k sample t falls in bin b(t) by pu_fold's rule, every step one IEEE float64 operation
 * and no fused multiply-add:
 *     p = phase0[k] + (double)(first_sample + t) * dphase[k]
 *     f = p - floor(p)
 *     b = min((int64)(f * (double)nbin), nbin - 1)
 * so host and device agree on every bin, edges included; a negative dphase, dphase = 0 and
 * |dphase| > 1 are all legal.  The call ACCUMULATES, as pu_fold does: sums[r * ld_row + k *
 * ld_trial + b] += the sum of (double)x[r][t] over the t with b(t) = b, counts[k * nbin + b] +=
 * their number (counts is shared by all rows; the caller zeroes both before the first chunk;
 * first_sample places a chunk, so the folds of the chunks of a long series add up).
 * Arithmetic: no floating-point atomics; the order of every sum is fixed by (n, first_sample,
 * phase0[k], dphase[k], nbin) alone: segments of 16384 samples from the chunk's start; inside
 * a segment, maximal runs of consecutive samples of one bin (cut at the segment's end), each
 * summed left to right; a bin's segment partial is 0.0 + its runs in time order; the partials
 * are added in segment order from segment 0's, then to sums.  Trial k's output bits depend
 * neither on ntrials, on k's position in the list, on rows nor on the device, and two equal
 * calls give equal bits.  Exact whenever the values and partial sums are integers below 2^53;
 * otherwise each call's addend to a bin is within m 2^-53 sum|x| of the exact sum of the bin's m
 * samples.  A non-finite phase0[k] or dphase[k], or |p| >= 2^52 at either end of the chunk,
 * cannot be rejected on the host without a synchronisation: such a trial gets NaN in all its
 * sums (every row) and leaves its counts unchanged; the other trials are not affected.
 * PU_EINVAL: nbin < 2; n < 0, rows < 0 or ntrials < 0; ld < n, ld_trial < nbin or ld_row <
 * ntrials * ld_trial; a workspace smaller than pu_fold_trials_workspace_bytes(rows, n, ntrials,
 * nbin) (rows x ceil(n / 16384) x ntrials x nbin x 8 bytes) or not 8-byte aligned.
 * PU_EUNSUPPORTED: nbin > 256 (a trial is a lane and its bins are LDS accumulators: 64 x nbin x
 * 8 bytes per wave within a budget of 144 KiB, next to 16 KiB of staged samples).  PU_OK without
 * a launch for n == 0, rows == 0 or ntrials == 0.  All checked before any HIP call; asynchronous
 * on stream. */
size_t pu_fold_trials_workspace_bytes(int64_t rows, int64_t n, int64_t ntrials, int64_t nbin);
int pu_fold_trials(const void *x, int dtype, int64_t rows, int64_t n, int64_t ld, int64_t first_sample,
                   const double *phase0, const double *dphase, int64_t ntrials, int64_t nbin,
                   double *sums, int64_t ld_trial, int64_t ld_row, int64_t *counts,
                   void *workspace, size_t workspace_bytes, void *stream);

/* The epoch-folding statistic of folded profiles of Gaussian-noise data (Leahy et al. 1983), on
 * pu_fold_trials' outputs.  With c_b = counts[k * nbin + b] and s_b = sums[r * ld_row + k *
 * ld_trial + b], for row r and trial k:
 *     chi2[r * ntrials + k] = sum over the b with c_b > 0 of (s_b - c_b mean[r])^2 / (c_b var[r])
 * accumulated sequentially over b in float64, one IEEE operation per step as written (no fused
 * multiply-add), and dof[k] = (the number of bins with c_b > 0) - 1.  mean, var: device [rows];
 * chi2: device [rows * ntrials]; dof: device [ntrials] int32.  var[r] not > 0 or a non-finite
 * s_b in any bin, empty ones included, gives NaN (so a trial pu_fold_trials filled with NaN
 * scores NaN, not 0).  (The H-test above is Poisson-normalised, P = sum p: not the statistic of
 * zero-mean noise.)  PU_EINVAL: nbin < 2, rows < 0 or ntrials < 0, ld_trial < nbin or ld_row <
 * ntrials * ld_trial; PU_OK without a launch for rows == 0 or ntrials == 0.  All checked before
 * any HIP call; asynchronous on stream. */
int pu_profile_chi2(const double *sums, int64_t ld_trial, int64_t ld_row, const int64_t *counts,
                    int64_t rows, int64_t ntrials, int64_t nbin, const double *mean, const double *var,
                    double *chi2, int32_t *dof, void *stream);

/* ------------------------------------------------------------------ FFT periodicity search */

/* Real-to-complex FFT of rows series: the first step of the blind periodicity search (no reference
 * counterpart).  x: device, rows series of n samples, leading dimension ld (PU_F32 / PU_F64; PU_U8
 * is PU_EUNSUPPORTED, as in pu_fold_trials).  mean: device float64 [rows], NULL means 0.  nfft: a
 * power of two, 2^8 <= nfft <= 2^24, n <= nfft.  For row r
 *     y[t] = (float)((double)x[r][t] - mean[r])   for t < n   (one float64 subtraction, one
 *            rounding to float32)
 *     y[t] = 0                                    for n <= t < nfft
 *     spec[r * ld_spec + k] = sum_t y[t] e^(-2 pi i k t / nfft),   k = 0 .. nfft / 2
 * as complex64 (float re, im), ld_spec >= nfft / 2 + 1 complex elements.  Arithmetic: float32,
 * no fused multiply-add, twiddles e^(-2 pi i k / nfft) rounded to float32 from float64
 * sincospi (a table at the start of the workspace, rebuilt by every call).  The half-length
 * complex transform of z[j] = y[2j] + i y[2j+1] runs in one LDS pass (nfft <= 2^13) or two
 * (four-step, nfft/2 = N1 x N2), radix-2 decimation in frequency, and a split step makes the
 * real-input spectrum in place in spec.  The order of every operation is fixed by nfft alone:
 * two equal calls give equal bits, and a row's bits depend neither on rows, on its position in
 * the batch nor on ld.  Error: the Cooley-Tukey bound, ||spec - exact||_2 <= 8 log2(nfft) 2^-24
 * ||exact||_2 per row (Higham, Accuracy and Stability of Numerical Algorithms, Thm 24.2).
 * workspace: pu_rfft_workspace_bytes(rows, nfft) bytes, 256-byte aligned: the twiddle table
 * (nfft / 2 complex64) and, above 2^13, rows x nfft / 2 complex64 between the two passes.
 * PU_EUNSUPPORTED: dtype.  PU_EINVAL: nfft not a power of two in [2^8, 2^24]; n < 0, n > nfft,
 * rows < 0 or > 65535; ld < n; ld_spec < nfft / 2 + 1; a NULL or misaligned pointer; a workspace too small
 * or not 256-byte aligned.  PU_OK without a launch for rows == 0.  All checked before any HIP
 * call; asynchronous on stream. */
size_t pu_rfft_workspace_bytes(int64_t rows, int64_t nfft);
int pu_rfft(const void *x, int dtype, int64_t rows, int64_t n, int64_t ld, const double *mean, int64_t nfft,
            void *spec, int64_t ld_spec, void *workspace, size_t workspace_bytes, void *stream);

/* Acceleration trials: time-domain resampling by nearest neighbour (the rule of peasoup and of
 * sigproc's seek), and pu_rfft with that index map applied where its first pass loads its
 * samples.  A signal of constant line-of-sight acceleration a is periodic again in the resampled
 * series.  afac: device float64 [nacc], the dimensionless factors af = a * sample_time / (2 c), c =
 * 299792458 m/s.  For a series of n samples (n <= 2^24) output sample i is input sample src(i):
 *     p   = (double)(i * (i - n))                  int64 product; exact
 *     q   = af * p                                 one float64 rounding, no fused multiply-add
 *     s   = fmin(fmax(rint(q), -(double)i), (double)(n - 1 - i))
 *     src = i + (int64)s
 * rint rounds ties to even; fmax and fmin drop a NaN.  The end points stay fixed, af = 0 is the
 * identity, and the clamp gives 0 <= src <= n - 1 for EVERY af (NaN and +-inf included): no input
 * makes a kernel read outside its row.  The map is monotone while |af| n <= 1.
 *
 * pu_resample_accel: out[(a * rows + r) * ld_out + i] = x[r * ld + src_a(i)], out of x's dtype
 * (PU_F32 / PU_F64), a plain gather; out must not overlap x.  PU_EUNSUPPORTED: dtype.  PU_EINVAL:
 * rows, nacc or n < 0, rows or nacc >= 2^31, n > 2^24; ld < n or ld_out < n; a NULL or misaligned
 * pointer; out == x.  PU_OK without a launch when rows, nacc or n is 0.
 *
 * pu_rfft_accel: pu_rfft over the nacc * rows virtual rows v = a * rows + r,
 *     y[t] = (float)((double)x[r][src_a(t)] - mean[r])   for t < n,   0 for n <= t < nfft
 * (the map takes n, not nfft), spec[v * ld_spec + k] as pu_rfft.  No resampled series is written:
 * everything after the load is pu_rfft's code, so the result has the bits of pu_rfft on
 * pu_resample_accel's output with the same mean (mean: [rows], NULL means 0), and at af = 0 the
 * bits of pu_rfft on x.  workspace: pu_rfft_accel_workspace_bytes(rows, nacc, nfft) = pu_rfft's
 * for nacc * rows rows.  Errors as pu_rfft with rows read as nacc * rows (at most 65535 per call);
 * also PU_EINVAL for rows or nacc < 0 or >= 2^31 and for a NULL or misaligned afac.
 * Both: all checked before any HIP call; asynchronous on stream. */
int pu_resample_accel(const void *x, int dtype, int64_t rows, int64_t n, int64_t ld, const double *afac,
                      int64_t nacc, void *out, int64_t ld_out, void *stream);
size_t pu_rfft_accel_workspace_bytes(int64_t rows, int64_t nacc, int64_t nfft);
int pu_rfft_accel(const void *x, int dtype, int64_t rows, int64_t n, int64_t ld, const double *mean,
                  const double *afac, int64_t nacc, int64_t nfft, void *spec, int64_t ld_spec, void *workspace,
                  size_t workspace_bytes, void *stream);

/* Power spectrum with the red noise taken out by a running median in blocks.  spec: device
 * complex64, rows x ld_spec (pu_rfft's output); nb = nfft / 2 bins k = 0 .. nb - 1 (the Nyquist
 * bin is dropped); block B: a power of two, 16 <= B <= min(1024, nb).  In float32, every step
 * one IEEE operation and no fused multiply-add:
 *     P[k] = re * re + im * im
 * Per block b (bins b B .. (b + 1) B - 1): s = the block's powers sorted ascending, with P[0]
 * replaced by +inf in block 0;
 *     med = 0.5f * (s[B/2 - 1] + s[B/2])      (block 0: med = s[B/2 - 1], the median of its
 *                                              B - 1 real bins)
 * If any power of the block is not finite (the replaced P[0] does not count) every output of
 * the block is NaN; otherwise if !(med > 0) every output is 0; otherwise
 *     out[r * ld_out + k] = P[k] * (0.6931472f / med)        (one division per block)
 * and out[r * ld_out + 0] = 0 always.  Noise then has mean about 1, each bin about Exp(1).
 * out: device float32, rows x ld_out, ld_out >= nb.  PU_EINVAL: nb not a power of two in [2^7,
 * 2^23], a bad block, rows < 0 or > 65535, ld_spec < nb, ld_out < nb, NULL pointers.  PU_OK without a
 * launch for rows == 0.  All checked before any HIP call; asynchronous on stream. */
int pu_spectrum_normalize(const void *spec, int64_t rows, int64_t nb, int64_t ld_spec, int64_t block,
                          float *out, int64_t ld_out, void *stream);

/* Incoherent harmonic sums of normalised spectra and their significant local maxima.  norm:
 * device float32, rows x ld (pu_spectrum_normalize's output), nb bins.  nlev levels, 1 <= nlev
 * <= 6; level l sums H = 2^l harmonics.  For every k in 0 .. nb - 1, in float32:
 *     S_0[k]     = norm[k]
 *     S_(l+1)[k] = S_l[k] + sum over odd m = 1, 3, .. 2H - 1 of norm[(k m + H) / (2H)],  H = 2^l
 * the terms added one at a time in ascending m to a running sum that starts at S_l[k]; the
 * division is an int64 division.  k is the bin of the TOP harmonic: the fundamental is at k / 2^l
 * bins.  sums (device, may be NULL: nothing is written): sums[l * ld_level + r * ld_row + k].
 * Candidates: thr (float32), kmin, kmax (int64): HOST arrays of nlev entries.  Bin k with kmin[l]
 * <= k < kmax[l] is a candidate of level l iff S_l[k] > thr[l], S_l[k] > S_l[k - 1] and S_l[k] >=
 * S_l[k + 1]; a neighbour outside [0, nb) counts as -inf; NaN compares false.  Candidates are
 * delivered sorted by (row, level, bin): *count (host) receives their number and the first
 * min(*count, cap) are written to cands (device; may be NULL when cap == 0: the call then only
 * counts).  Count, scan and fill kernels with integer arithmetic only: the order and the total
 * do not depend on timing.  workspace: pu_harmonic_search_workspace_bytes(rows, nb, nlev),
 * 256-byte aligned.  PU_EINVAL: nlev outside [1, 6], rows < 0 or > 65535, nb < 1 or > 2^23, ld <
 * nb, bad strides of sums, cap < 0, NULL pointers, a workspace too small or misaligned.  All
 * checked before any HIP call.  The call synchronises the stream once (as pu_series_events). */
typedef struct pu_spec_cand {
    int32_t row, level;
    int64_t bin;
    float power, pad;
} pu_spec_cand;
size_t pu_harmonic_search_workspace_bytes(int64_t rows, int64_t nb, int64_t nlev);
int pu_harmonic_search(const float *norm, int64_t rows, int64_t nb, int64_t ld, int64_t nlev, float *sums,
                       int64_t ld_level, int64_t ld_row, const float *thr, const int64_t *kmin,
                       const int64_t *kmax, pu_spec_cand *cands, int64_t cap, int64_t *count,
                       void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ fast folding (FFA) */

/* The fast folding algorithm: all m trial periods between p and p + 1 bins of a series of m x p
 * samples for n log2 m adds, and the boxcar matched-filter S/N of the folded profiles.  No
 * reference counterpart; the definition is this project's own (tests/ffa_oracle.py restates it in
 * numpy) and claims parity with no other package.
 *
 * rdiv(a, b) = (2a + b) / (2b) for non-negative integers (integer division): a / b rounded half up.
 *
 * Transform.  The input is m >= 1 rows of p >= 2 float32 bins, x[i][j] = series[i p + j]; F(x) has
 * m rows.  For m = 1, F(x) = x.  Otherwise nh = m / 2 (integer), nt = m - nh, H = F(x[0 .. nh)),
 * T = F(x[nh .. m)), and for s = 0 .. m - 1
 *     h = rdiv(s (nh - 1), m - 1),   t = rdiv(s (nt - 1), m - 1),   b = s - t
 *     F[s][j] = H[h][j] + T[t][(j + b) mod p]
 * each add one float32 addition with the head operand on the left, nothing fused or reassociated:
 * every output bit is fixed by (m, p) and the row's samples alone, and numpy reproduces it.  Row s
 * folds at a period of p + s / (m - 1) bins (p for m = 1); row 0 is the plain fold; row m - 1
 * shifts input row i by exactly i, the period of row 0 at base period p + 1.  In between, the
 * shift the tree gives input row i in trial s is non-decreasing in i and within 3 bins of
 * s i / (m - 1) (checked for m = 2 .. 1099, 2048, 4096, 4099: worst 2.96, worst per-trial rms
 * 1.43, about 0.35 for powers of two, where the rule is the classic radix-2 FFA).
 *
 * S/N.  For the profile v = F[s] (float32), a width w with 1 <= w < p and the noise sigma[r] of the
 * series (device float64 [rows]; NULL means 1):
 *     T   = sum_j (double)v[j]
 *     B_w = max over b = 0 .. p - 1 of sum_{i < w} (double)v[(b + i) mod p]
 *     snr = (float)((B_w - w T / p) / (sqrt((double)m w (1 - (double)w / p)) sigma[r]))
 *     peak = the lowest b whose computed sum attains the maximum
 * The sums are float64 differences of float64 prefix sums (a wave scan per 64 bins).  Bound: with
 * A = sum_j |v[j]|, every computed window sum and the computed T are within 4 p 2^-53 A of their
 * exact values, so the numerator is within N = 8 p 2^-53 A of the exact one and
 *     |snr - exact| <= N / (sqrt(m w (1 - w / p)) sigma[r]) + 2^-23 |exact|
 * (the last term: the quotient's float64 roundings and the one rounding to float32, barring
 * underflow), and the exact window sum at the reported peak is within N of the exact maximum.
 * Integer-valued samples whose sums stay below 2^24 make every sum exact.  A non-finite sample
 * gives unspecified snr and peak in the trials that read it and touches no other.
 *
 * pu_ffa.  x: device, rows series; samples 0 .. m p - 1 of each are read and nothing beyond, ld >=
 * m p.  out (device, may be NULL): out[r ld_out_row + s p + j] = F[s][j]; only those m p elements
 * of a row are written.  snr (device, may be NULL): snr[(r m + s) nwidths + k] = the S/N at width
 * widths[k]; peak (device int32, optional, only with snr): the same layout.  widths: a HOST array of
 * nwidths int32, validated here and passed to the kernel by value (no device copy, no
 * synchronisation).  The bottom levels run in LDS, B = pu_ffa_describe's "block_rows" rows per
 * workgroup; the others are one pass over the plane each.  With out == NULL the top level is
 * formed inside the S/N kernel and never written (when the tree has a level above the LDS ones);
 * snr and peak have the same bits either way.  workspace: pu_ffa_describe's "workspace_bytes",
 * 256-byte aligned (none when out is given and m <= B).  Two equal calls give equal bits; a row's
 * bits depend neither on rows nor on its position in the batch.
 * PU_EINVAL: p < 2; m < 1; rows < 0; ld < m p; ld_out_row < m p (with out); both out and snr NULL;
 * peak without snr; with snr, nwidths outside 1 .. 16, a NULL widths or a width outside 1 .. p - 1;
 * a NULL x or a misaligned pointer; a workspace too small or not 256-byte aligned.
 * PU_EUNSUPPORTED: p > 2048 (an LDS block is two buffers of B p floats, B >= 8, within 128 KiB);
 * rows x m > 2^31 - 1 (the grid of one call: the caller batches rows).  PU_OK without a launch for
 * rows == 0.  All checked before any HIP call; asynchronous on stream.
 *
 * pu_ffa_describe: host only, no HIP call; what pu_ffa would do for the same sizes (want_out: out
 * != NULL; nwidths: 0 when snr == NULL).  Fills up to n of {depth = ceil(log2 m), lds_levels,
 * block_rows (B: the largest power of two <= 256 with B p <= 16384, whatever m is), workspace_bytes,
 * global_levels (depth - lds_levels), p_max, lds_bytes (of the LDS kernel's workgroup),
 * traffic_bytes (what the level split moves through device memory: the LDS kernel reads the
 * series and writes a plane, every level above reads one plane and writes one - none when the top
 * level is fused -, an unfused S/N reads one; plus snr and peak)}.  Errors as pu_ffa's for rows,
 * m, p; nwidths outside 0 .. 16 or nothing wanted: PU_EINVAL. */
int pu_ffa_describe(int64_t rows, int64_t m, int64_t p, int64_t nwidths, int want_out, int64_t *info, int n);
int pu_ffa(const float *x, int64_t rows, int64_t ld, int64_t m, int64_t p, float *out, int64_t ld_out_row,
           const int32_t *widths, int64_t nwidths, const double *sigma, float *snr, int32_t *peak,
           void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ running-median detrending */

/* A sliding-window median and the baseline built from it, to take red noise out of a time series
 * before it is folded.  No reference counterpart; the definition is this project's own
 * (tests/detrend_oracle.py restates it in numpy) and claims parity with no other package.  Every
 * output bit is fixed by the arguments: no floating-point atomics, nothing depends on timing, on
 * rows or on a row's position in the batch.
 *
 * Running median.  The width w is odd, h = (w - 1) / 2.  out[r][i] is the median of the w values
 * x[r][clip(i + k, 0, n - 1)], k = -h .. h: the edge sample is repeated (scipy.ndimage's
 * median_filter, mode "nearest").  The median of an odd count is an element of the window: no
 * arithmetic.  Order: by value, -0 before +0; +-inf are ordinary values.  A window that holds any
 * NaN gives the canonical quiet NaN (0x7fc00000, 0x7ff8000000000000), the rule np.median follows.
 *
 * Plan.  A width of W samples and min_points (101) give the block length d = max(1, W /
 * min_points) and the median width w = 2 ((W / d) / 2) + 1 (integer divisions): the median runs
 * over between min_points and 2 min_points block means, whatever W is.
 *
 * Baseline.  nblk = n / d >= 1 blocks; sum[b] is pu_rebin_time's float64 sum of block b (d samples
 * added in order to 0.0), mean[b] = sum[b] / (double)d, med = the running median of mean at width
 * w.  For sample i, in float64, every step one IEEE operation and nothing fused:
 *     u    = (double)(2 i - d + 1) / (double)(2 d)       (block centres sit at u = 0, 1, 2 ..)
 *     b0   = clip(floor(u), 0, nblk - 2)
 *     t    = clip(u - b0, 0, 1)
 *     base = med[b0] + t (med[b0 + 1] - med[b0])       for 0 < t < 1
 *     base = med[b0] for t == 0, med[b0 + 1] for t == 1  (the median itself: m0 + (m1 - m0) need not be m1)
 * and base = med[0] for nblk == 1.  So samples up to the first block centre take med[0] and samples
 * from the last one on take med[nblk - 1], the n - nblk d samples of the tail among them, in every
 * bit; for d == 1 base is med.
 *     out[i] = (T)((double)x[i] - base)
 * A NaN in med reaches exactly the samples that take it with a weight above 0; the sign and
 * payload of a NaN that this arithmetic makes are unspecified.
 *
 * pu_running_median.  x, out: device, rows of n elements of dtype (PU_F32 or PU_F64, the same for
 * both), ld >= n and ld_out >= n elements apart; they must not overlap.  A workgroup stages its
 * tile of outputs plus the 2h halo, edge-clamped, in LDS as order-preserving unsigned keys and
 * selects each output by a radix descent over the key bits, most significant first; no workspace.
 * Only the n elements of a row of out are written.
 * PU_EUNSUPPORTED: another dtype; w > 2047; rows x tiles above 2^31 - 1.  PU_EINVAL: rows < 0,
 * n < 1, ld < n, ld_out < n, w < 1 or even; a NULL or misaligned pointer; rows that run beyond the
 * address space; overlapping x and out.
 * PU_OK without a launch for rows == 0.  All checked before any HIP call; asynchronous on stream.
 *
 * pu_running_median_describe: host only, no HIP call.  Fills up to n of {tile (outputs of a
 * workgroup), lds_bytes (of a workgroup at this dtype and w), w_max (2047)}.  Errors as
 * pu_running_median's for dtype and w; a NULL info or n < 0: PU_EINVAL.
 *
 * pu_detrend_apply.  x: device, rows of n elements of dtype (PU_F32 or PU_F64), ld >= n; med:
 * device float64, rows of nblk medians, ld_med >= nblk; out: the dtype of x, ld_out >= n, and may
 * be x itself (the same pointer and ld_out == ld; any other overlap is refused): the operation is elementwise, one read and one write per
 * sample, 16 bytes per lane where x, out and both strides are aligned to that.
 * PU_EUNSUPPORTED: another dtype; n above 2^51; rows x n / 256 above 2^31 - 1.  PU_EINVAL:
 * rows < 0, n < 1, d < 1, nblk < 1, nblk != n / d, ld < n, ld_out < n, ld_med < nblk; a NULL or
 * misaligned pointer; rows that run beyond the address space; out overlapping x without being x.  PU_OK without a launch for rows == 0.  All checked before any HIP call;
 * asynchronous on stream. */
int pu_running_median_describe(int dtype, int64_t w, int64_t *info, int n);
int pu_running_median(const void *x, int dtype, int64_t rows, int64_t n, int64_t ld, int64_t w, void *out,
                      int64_t ld_out, void *stream);
int pu_detrend_apply(const void *x, int dtype, int64_t rows, int64_t n, int64_t ld, const double *med,
                     int64_t ld_med, int64_t nblk, int64_t d, void *out, int64_t ld_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PULSARUTILS_HIP_H */
