/* rt_frontend.h — C ABI of the MI355X analog front end (librtfe.so).
 *
 * The drop-in boundary.  The reference (LenShustek/readtape V3.18) has no plugin or FFI surface;
 * its de-facto seam is   bool readblock(bool retry)            src/readtape.c:1396
 * which loops            enum bstate_t process_sample(...)     src/decoder.c:817 (decl. src/decoder.h:384)
 * and, beneath it, the callback set the front end drives:
 *        void {nrzi,pe,gcr,ww}_{top,bot}(struct trkstate_t*)   src/decoder.h:385-399
 * after  init_trackstate()                                     src/decoder.c:425.
 * This library replaces everything between those two seams: given the TBIN payload resident in HBM
 * it produces, per block attempt and per parameter set, exactly the sequence of top/bot calls the
 * reference's process_sample() would make (track, polarity, peak time, voltage, detection sample,
 * AGC gain), as 16-byte event records.  INTEGRATION.md shows the reference-side stub.
 *
 * Plain pointers and sizes only; every pointer whose name starts with d_ is a DEVICE pointer
 * (hipMalloc / torch storage).  All calls are asynchronous on `stream` (a hipStream_t passed as
 * void*, NULL = default stream) unless stated; nothing here synchronises the device.  (rtfe_scan may run one of
 * its kernels - the burst heads - on a stream of its own beside the dense pass; it forks from and joins back into
 * `stream` with events, so everything rtfe_scan wrote is complete when `stream` reaches the point behind the call.)
 *
 * Exactness contract.  The reference restarts all detector state at every block attempt
 * (src/decoder.c:425-455), at a sample only its sequential bit decoders know.  rtfe_scan()
 * speculates: it restarts inside every inter-block quiet zone ("burst" boundary) and reports, per
 * burst, the interval [zone_first, safe_last] of restart samples for which its output is PROVABLY
 * identical to the reference's (dead-quiet signal, full windows, common min/max rescan — see
 * DESIGN.md §3).  A caller whose true restart sample falls outside the interval, or whose block
 * does not end inside a zone, calls rtfe_scan_exact() for that one attempt: same kernels, caller-
 * given restart sample, no speculation.  Neither path computes anything on the CPU.
 */
#ifndef RT_FRONTEND_H
#define RT_FRONTEND_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTFE_MAXTRKS     19   /* src/csvtbin.h:29  MAXTRKS      */
#define RTFE_MAXPARMSETS 15   /* src/decoder.h:92  MAXPARMSETS  */
#define RTFE_ABI_VERSION 6   /* 6: rtfe_reset_floor (a handle's first scan estimates the candidate screen's floor from the samples); 5: rtfe_set_graphs; 4: rtfe_pack_events; 3: rtfe_scan_stats out[21] = the smallest learned peak height (screen-floor calibration); 2: rtfe_kernel_ms returns the number of scans summed; twelve timed spans (k_dseg, k_dchain) */

enum { RTFE_PE = 1, RTFE_NRZI = 2, RTFE_GCR = 4, RTFE_WW = 8 };      /* enum mode_t, src/csvtbin.h:47-49 */

/* the front-end half of struct parms_t (src/decoder.h:290-310) */
typedef struct rtfe_parmset {
   float   pkww_bitfrac;     /* window width as a fraction of a bit cell              */
   float   pkww_rise;        /* required rise, volts at 4 V p-p                       */
   float   min_peak;         /* absolute minimum peak, volts (0 = none)               */
   float   agc_alpha;        /* exponential AGC weight (0 = off)                      */
   int32_t agc_window;       /* min-of-last-n AGC window (0 = off)                    */
   float   clk_factor;       /* PE only: clock window factor (decides preamble end)   */
} rtfe_parmset;

typedef struct rtfe_config {
   int32_t mode;                          /* RTFE_NRZI ...                                        */
   int32_t ntrks;                         /* tracks == heads in a TBIN row                        */
   int32_t head_to_trk[RTFE_MAXTRKS];     /* column -> track permutation (src/readtape.c:1419)    */
   int32_t invert;                        /* -invert        (src/readtape.c:1421)                 */
   int32_t differentiate;                 /* -differentiate (src/readtape.c:1383-1388)            */
   int32_t find_zeros;                    /* -zeros         (src/decoder.c:863-865)               */
   int32_t skew_delaycnt[RTFE_MAXTRKS];   /* -skew=n,n,..   in samples (src/decoder.c:232)        */
   float   maxvolts;                      /* TBIN header                                          */
   float   bpi, ips;                      /* bpi = 0: density unknown -> the front end of the reference's density pre-pass
                                           * (window of 8 samples, no AGC feedback; src/readtape.c:1457,1656-1672; NRZI peaks only) */
   int64_t tdelta_ns;                     /* sample period                                        */
   int64_t tstart_ns;                     /* time of row 0                                        */
   int32_t nparmsets;
   rtfe_parmset parmset[RTFE_MAXPARMSETS];
   /* speculation / screening knobs (performance only; results are exact or flagged) */
   int32_t gap_min_samples;               /* quiet run treated as an inter-block gap; 0 = 32 bit cells */
   float   quiet_volts;                   /* |v| band of the dead-quiet test; 0 = default         */
   float   screen_floor_height;           /* assumed lower bound of the AGC baseline (v_avg_height) for
                                             the candidate screen.  A burst whose measured baseline is lower is
                                             flagged RTFE_F_SCREEN_UNDERFLOW.  0 = the handle follows the tape: its first
                                             scan of the peak path estimates the floor from the samples before it screens
                                             (0.45 x the smallest peak-to-peak range inside a block; 1.0 V where it finds
                                             no block), and behind each scan the floor moves to half the smallest peak
                                             height the scan's chains learned (rtfe_scan_stats out[22]; rtfe_reset_floor) */
   float   events_per_sample_cap;         /* per-track event capacity as a fraction of the burst length;
                                             0 = default 1/8 */
} rtfe_config;

/* One flux-transition event = one call of {mode}_top/_bot in the reference (src/decoder.c:574-609). */
typedef struct rtfe_event {
   uint32_t sample;          /* detection sample (the reference's `timenow` row), relative to the burst's reset_sample */
   float    v_peak;          /* t->v_top / t->v_bot, volts                                          */
   float    agc_gain;        /* t->agc_gain when the callback is entered                            */
   uint8_t  trk;
   uint8_t  flags;           /* bit0: 0 = top (up transition), 1 = bottom; bits 1-2: time adjustment
                                code 0 = none, 1 = -0.5 sample, 2 = +0.5 sample (src/decoder.c:718-730).
                                bit 7 (RTFE_EV_FATAL): not a transition - at this row the reference's
                                "AGC gain bad in lookfor_peak" assert (src/decoder.c:782) fires on this track,
                                which ends the whole run there (exit 99); nothing follows it on the track */
   uint8_t  left_distance;   /* 1-based position of the peak in the window (src/decoder.c:704-744)  */
   uint8_t  parmset;
} rtfe_event;                /* 16 bytes */

/* peak time exactly as refine_peak forms it (src/decoder.c:732); W = pkww_width of the parmset:
 *   timenow = (double)(tstart_ns + (reset_sample + sample) * tdelta_ns) / 1e9
 *   t_peak  = timenow - ((float)(W - left_distance) - adj) * sample_deltat          */

enum {
   RTFE_F_EXACT_START      = 1,    /* reset_sample was given by the caller (or is row 0)             */
   RTFE_F_UNSAFE           = 2,    /* no provably-equivalent restart interval exists for this burst  */
   RTFE_F_EVENT_OVERFLOW   = 4,    /* a track's event region filled up; events were dropped          */
   RTFE_F_SCREEN_UNDERFLOW = 8,    /* AGC threshold fell below the candidate screen: rescan exactly with screen off */
   RTFE_F_TRUNCATED        = 32,   /* time shard: the halo ended before this burst's successor zone did          */
   RTFE_F_DETECTOR_FATAL   = 16,   /* the reference would have hit its fatal "peak at window edge" assert (src/decoder.c:709-710,748) */
   RTFE_F_AGC_FATAL        = 128,  /* informational: a track's event list ends in an RTFE_EV_FATAL marker                     */
   RTFE_F_STATE_AT_END     = 64    /* -zeros: at end_sample a track still holds an excursion beyond the 0.2 V threshold or a pending
                                    * crossing - history a restart would not have, even if no event was emitted: an attempt that
                                    * reaches the end of this burst must not continue into the next one */
};

#define RTFE_EV_FATAL 0x80

typedef struct rtfe_burst {
   int64_t  zone_first;      /* first row of the dead-quiet zone that precedes this burst            */
   int64_t  zone_end;        /* one past the last row of that zone                                    */
   int64_t  reset_sample;    /* row at which this burst's detector state was restarted                */
   int64_t  safe_last;       /* any true restart row in [zone_first, safe_last] gives identical events */
   int64_t  end_sample;      /* rows [reset_sample, end_sample) were scanned with this burst's state  */
   uint64_t event_base;      /* index into the event buffer of this burst's first region              */
   uint32_t event_cap;       /* capacity of each (parmset, track) region                              */
   uint32_t flags;           /* RTFE_F_*                                                              */
} rtfe_burst;                /* 56 bytes */
/* region of (burst b, parmset p, track t):  events[ b.event_base + (p * ntrks + t) * b.event_cap ... ],
 * count in counts[(burst_index * nparmsets + p) * ntrks + t]; events of one region are in detection order. */

typedef struct rtfe_handle rtfe_handle;

int         rtfe_abi_version(void);
const char *rtfe_last_error(void);

/* Validates the configuration and precomputes window widths, thresholds and the candidate screen.
 * Returns 0 or a negative error (message via rtfe_last_error). Synchronous, no device work. */
int  rtfe_create(const rtfe_config *cfg, rtfe_handle **out);
void rtfe_destroy(rtfe_handle *h);
int  rtfe_pkww_width(const rtfe_handle *h, int parmset);      /* src/readtape.c:1455-1457 */

/* The path rtfe_scan takes for this handle, as rtfe_create decided it from the configuration and the environment knobs:
 *   RTFE_PATH_PEAK       k_sift -> k_gain -> k_emit (NRZI peak detection)
 *   RTFE_PATH_DENSE      k_dseg -> k_dchain (PE, GCR peak detection)
 *   RTFE_PATH_ZEROS      k_zeros (-zeros)
 *   RTFE_PATH_DIFFZEROS  k_diffz (-zeros -differentiate)
 *   RTFE_PATH_SAMPLE     k_decode, a lane per (parameter set, track) on the samples: everything else, and what the knobs send there
 *   RTFE_PATH_WW         Whirlwind: rtfe_scan refuses, rtfe_ww_scan / rtfe_ww_detector_scan serve the handle
 * What a caller sizes its expectations by (the sample path is one to two orders of magnitude slower per row); the events do not depend on it. */
enum { RTFE_PATH_PEAK, RTFE_PATH_DENSE, RTFE_PATH_ZEROS, RTFE_PATH_DIFFZEROS, RTFE_PATH_SAMPLE, RTFE_PATH_WW };
int  rtfe_detector_path(const rtfe_handle *h);

/* Sizes the caller must provide for a scan of nrows rows. */
size_t  rtfe_workspace_bytes(const rtfe_handle *h, int64_t nrows);
int64_t rtfe_max_bursts(const rtfe_handle *h, int64_t nrows);
int64_t rtfe_event_capacity(const rtfe_handle *h, int64_t nrows);

/* Speculative scan of d_rows[0 .. nrows) (interleaved int16, ntrks per row, the TBIN payload).
 * Time shards: row_base is the absolute index of d_rows[0] on the tape (used for times only; all rows in
 * the outputs are relative to d_rows[0]); first_is_tape_start says row 0 is a true restart point (the
 * start of the tape); own_rows <= nrows is the part of the slice this scan OWNS — rows
 * [own_rows, nrows) are the halo received from the right neighbour.  Zones are found on whole groups of 64
 * rows: a group is quiet iff it is complete and every sample of every track lies inside the quiet band, a
 * zone is a maximal run of at least G quiet groups (G = the gap length in groups, rtfe_max_bursts(h, n) ==
 * (n / 64) / G + 4), zone_first = 64 * its first group, zone_end = 64 * (its last group + 1).  The rows of an
 * incomplete last group are never quiet, so a zone that ends with the tape ends at nrows rounded down to a
 * multiple of 64 and zone_end <= nrows always.  A burst is decoded here iff its zone_end < own_rows + 64 G:
 * a zone that reaches G groups or more past own_rows qualifies in the right neighbour's slice (whose row 0
 * is own_rows) and is decoded there, one that ends earlier shows the neighbour too few quiet groups and
 * stays here; the exact-start burst of row 0 (first_is_tape_start, and the slice does not begin with G quiet
 * groups) is always owned.  The last owned burst runs on into the halo up to the next zone's restart row;
 * that next burst's entry is written at bursts[*nbursts] as k_bursts made it (reset_sample = safe_last = -1,
 * end_sample provisional); what lies behind it means nothing.  If the halo holds no further zone the last owned burst is
 * flagged RTFE_F_TRUNCATED (pass a longer halo).  own_rows == nrows: no halo (single GPU, or the last shard).
 * Event regions: event_cap = (int)((float)len * cap) + 64 in float32, len = the rows from zone_end - 256 (an
 * exact-start burst: row 0) to the next table entry's zone_end (the last entry: nrows), cap = events_per_sample_cap;
 * event_base = the sum, over the bursts in front, of a burst's nparmsets * ntrks regions rounded up to 64 events.  A burst whose regions would pass
 * event_capacity gets event_cap = 0 and RTFE_F_EVENT_OVERFLOW; the bases behind it go on as if it had fitted.
 * Outputs (device): bursts[*nbursts] (owned bursts only), counts, events. */
int rtfe_scan(rtfe_handle *h, const int16_t *d_rows, int64_t nrows, int64_t own_rows, int64_t row_base, int first_is_tape_start,
              void *d_workspace, size_t workspace_bytes,
              rtfe_burst *d_bursts, int64_t max_bursts, int32_t *d_nbursts,
              uint32_t *d_counts, rtfe_event *d_events, int64_t event_capacity,
              void *stream);

/* The scans of ONE handle read and move its device-resident screen (above): queue them on one stream, or order the streams yourself.
 * rtfe_reset_floor: the screen back to what rtfe_create made (queued on `stream`) - the next scan is a tape's first scan again (a new tape on an old
 * handle; bench.py's "...f" lines time exactly that). */
int rtfe_reset_floor(rtfe_handle *h, void *stream);

/* Exact scan of one block attempt: detector state restarts at `reset_row` (index into d_rows) and
 * rows [reset_row, end_row) are scanned; parmset_mask selects parameter sets.  With screen_off != 0
 * every sample is examined (use after RTFE_F_SCREEN_UNDERFLOW).  Writes one rtfe_burst. */
int rtfe_scan_exact(rtfe_handle *h, const int16_t *d_rows, int64_t nrows, int64_t row_base,
                    int64_t reset_row, int64_t end_row, uint32_t parmset_mask, int screen_off,
                    void *d_workspace, size_t workspace_bytes,
                    rtfe_burst *d_burst, uint32_t *d_counts, rtfe_event *d_events, int64_t event_capacity,
                    void *stream);

/* The event lists of a scan, packed on the device (what crosses PCIe to the host replay: the arena is laid out for the worst case, event_cap
 * records per list; the lists hold a fraction of it).  Queued on `stream` behind the rtfe_scan whose outputs it reads:
 *   d_plan[b], b < *d_nbursts: burst b's lists in d_packed under the burst table's own addressing rule -
 *     d_packed[plan.event_base + (p * ntrks + t) * plan.event_cap + i], plan.event_cap = the burst's longest list (>= 1);
 *   d_plan[*d_nbursts].event_base = records of d_packed in use (.reserved = the burst count the plan was made for).  If that exceeds
 *     packed_capacity nothing was copied: fetch the arena as it is, or pack again into a larger buffer.
 * d_plan holds max_bursts + 1 entries.  The scan's own outputs are not changed. */
typedef struct rtfe_pack_entry { uint64_t event_base; uint32_t event_cap; uint32_t reserved; } rtfe_pack_entry;      /* 16 bytes */
int rtfe_pack_events(rtfe_handle *h, const rtfe_burst *d_bursts, const int32_t *d_nbursts, int64_t max_bursts, const uint32_t *d_counts,
                     const rtfe_event *d_events, rtfe_event *d_packed, uint64_t packed_capacity, rtfe_pack_entry *d_plan, void *stream);

/* The end of the data inside a window of the payload: *d_first = the first row of d_rows[0 .. nrows) whose head-0 sample is 0x8000 (the reader of
 * src/readtape.c:1410 stops there), INT64_MAX if there is none.  Queued on `stream`; a streaming reader runs it behind a window's upload instead of
 * passing over the window on the host. */
int rtfe_find_end_mark(rtfe_handle *h, const int16_t *d_rows, int64_t nrows, int64_t *d_first, void *stream);

/* -subsample on a raw window (src/readtape.c:1407-1424: of every n rows the reader uses the last one, but looks for the end marker on all of them).
 * Handle-free and queued on `stream`: no host synchronisation, no allocation.  The ABI version did not move: an addition, and rtfe_kernel_count() stays
 * what it was (this kernel is no span of a scan).
 *   d_out row j = d_in row first + j * step, for every j with first + j * step < nrows_in (rows of ntrks int16; step 1 is a plain copy);
 *   *d_first_mark = rtfe_find_end_mark's answer over the RAW rows: the smallest row of d_in[0 .. nrows_in) whose head-0 sample is 0x8000, INT64_MAX if there
 *   is none - the skipped rows and the rows in front of `first` included, and also when there is no row to write.
 * The kernel does not clip at the marker: the caller keeps row j iff first + j * step < *d_first_mark (a group of `step` rows that the marker cuts short is
 * dropped, as the reader drops it).  A streaming reader calls it with first = step - 1 between a window's upload and its rtfe_scan, in place of
 * rtfe_find_end_mark.
 * Memory contract: reads exactly the bytes of d_in[0 .. nrows_in) - none behind the last source row, the window's last, partial 16-byte vector is fetched
 * sample by sample - and writes exactly the bytes of the rows listed above and the 8 bytes of *d_first_mark: none in front of d_out, none behind its last
 * written row (that row's partial 16-byte vector is stored sample by sample).
 * Refusals, all before anything is queued (d_out and *d_first_mark are left alone): a null pointer: -1; ntrks outside 1 .. 19: -3; step < 1, first < 0,
 * nrows_in < 0 or more rows than a launch takes: -34; d_in or d_out not 16-byte aligned: -31; out_cap_rows smaller than the rows to write: -32; the byte
 * ranges of d_in[0 .. nrows_in) and of the rows to write overlap (in place is not supported): -37.  rtfe_last_error says which.
 * rtfe_decimate_span_rows(ntrks): the raw rows one workgroup (one wave) of the kernel takes - a multiple of 8; for tests and tools that aim at its seams. */
int64_t rtfe_decimate_span_rows(int ntrks);
int rtfe_decimate_rows(const int16_t *d_in, int64_t nrows_in, int ntrks, int64_t first, int64_t step, int16_t *d_out, int64_t out_cap_rows,
                       int64_t *d_first_mark, void *stream);

/* Per-kernel timing: with enable != 0, rtfe_scan records HIP events on `stream` around each of its timed spans (rtfe_kernel_name), one
 * set of events per scan in a ring of 64 sets - nothing waits, so scans queued back to back stay back to back.  rtfe_kernel_ms synchronises
 * the sets recorded since its last call and returns, per span, the elapsed milliseconds SUMMED over those scans (out[rtfe_kernel_count()]);
 * its return value is the number of scans summed (>= 0), or a negative error.  A span a scan did not run adds exactly 0 for that scan.  Used by bench.py. */
int rtfe_set_timing(rtfe_handle *h, int enable);

/* HIP graphs (ABI 5).  enable != 0: rtfe_scan captures its launches - about twenty kernels and memsets on the caller's stream and a stream of the handle's
 * own - into a hipGraph the first time it meets a set of arguments (pointers, sizes, flags) and replays that graph for every later scan with the same
 * arguments: one launch on the host, no gaps between the kernels on the device.  The handle keeps the eight most recently used graphs (a streaming reader's
 * ring of windows).  Results are the same either way.  Scans on the legacy default stream (stream == NULL), with per-kernel timing on or with debug
 * counters are launched directly; so is everything if the runtime refuses the capture.  The buffers a graph names must stay allocated while scans with
 * those arguments may still come; rtfe_destroy frees the graphs.  Environment default: RTFE_GRAPHS. */
int rtfe_set_graphs(rtfe_handle *h, int enable);
int rtfe_kernel_ms(rtfe_handle *h, float *out);

/* Statistics of the most recent rtfe_scan that used d_workspace (synchronous, call after the stream has finished):
 * out[0] = bursts decoded, out[1] = of which the record chains handed to the exact sample path, out[2] = bytes of peak
 * records written, out[3] / out[4] = detections the chains decided 64 runs at a time / one at a time.  Diagnostics for bench.py
 * and the tests; no effect on results.  out[5..12] = chains that gave up, by reason; out[13..20] = cycle counters of k_sift / k_gain / k_bursts / k_gain_seg (RTFE_DEBUG=3 / 4 / 5 / 6).
 * out[21] = 0x7fffffff - the IEEE bits of the smallest v_avg_height (src/decode_nrzi.c:224-229) a chain of the scan learned, 0 if none did (peak path):
 * what a caller may raise rtfe_config::screen_floor_height towards for the next scans of the same tape - a floor above a later chain's learned height is
 * flagged RTFE_F_SCREEN_UNDERFLOW and costs an exact rescan, never a wrong event.  out[22] = the IEEE bits of the floor the handle's next scan screens against:
 * with rtfe_config::screen_floor_height == 0 the handle's first scan estimates it from the samples and every scan of the peak path moves it, behind itself, to half
 * the smallest height its chains learned (on the device, nothing waits; a floor the caller gives stands).  out[23] = the IEEE bits of the floor THIS scan's screen was built for (peak path).
 * out must hold 24 values. */
int rtfe_scan_stats(rtfe_handle *h, const void *d_workspace, int64_t *out);

/* Names and launch-order of the kernels of one scan, for profilers (static strings). */
int         rtfe_kernel_count(void);
const char *rtfe_kernel_name(int i);

/* ---- Whirlwind (mode RTFE_WW): detector state that survives block attempts ----
 * The reference never restarts its detector between Whirlwind blocks (src/readtape.c:1674, src/decode_ww.c:31-49); a new attempt
 * only re-seeds every track's window (ring slot 0 and both extremes, src/decoder.c:855-861), one track per sample.  Where an
 * attempt starts is the host decoder's decision, so the host hands the state in and gets it back:
 *   rtfe_ww_scan: rows [first_row, first_row + nscan) of d_rows from the state d_state_in (one rtfe_ww_track per track; a tape
 *   starts from rtfe_ww_initial_state), the attempt they belong to having started at seed_row0 (<= first_row: track t sits out
 *   rows < seed_row0 + t and is re-seeded at seed_row0 + t).  Out: per-track event lists (event.sample relative to first_row;
 *   d_events[t * event_capacity ...], d_counts[t]), the state after the last row (d_state_out, may alias d_state_in), *d_flags |=
 *   RTFE_F_* conditions.  One parameter set (the reference forbids -m for Whirlwind), peak detection only.  -deskew: the reference
 *   learns the delays AND the pulse heights in a pre-pass over the first blocks, then clears the windows and starts over
 *   (src/readtape.c:1676-1716): the host replay does the same with this call - pre-pass from the initial state, then left/right/
 *   maxv/minv/countdown = 0, v_avg_height and delay set per track in the blob, and the decode from row 0.
 * Replaces: the per-sample lookfor_peak of src/decoder.c:751-810 for mode WW, at the seam of src/decoder.c:586,604. */
typedef struct rtfe_ww_track {
   int16_t ring[64];                /* pkww_v as int16 codes (after -invert; there -32768 stands for +32768, the inverted -32768) */
   int32_t left, right, maxv, minv, countdown, peakcount, heightndx;
   int32_t delay;                   /* -deskew: this track's delay in samples (0..50; the FIFO of src/decoder.c:820-830 starts at row 0 of the tape) */
   float   agc_gain, v_avg_height, v_lasttop, v_lastbot, v_top, v_bot;
   float   heights[10];
} rtfe_ww_track;                     /* 224 bytes */
void rtfe_ww_initial_state(rtfe_ww_track *tracks, int ntrks);        /* init_trackstate, src/decoder.c:425-455 (host memory) */
int rtfe_ww_scan(rtfe_handle *h, const int16_t *d_rows, int64_t nrows, int64_t row_base, int64_t first_row, int64_t nscan, int64_t seed_row0,
                 const rtfe_ww_track *d_state_in, rtfe_ww_track *d_state_out, uint32_t *d_counts, rtfe_event *d_events, int64_t event_capacity,
                 uint32_t *d_flags, void *stream);

/* ---- Whirlwind with -zeros and / or -differentiate: the other three detectors, same contract ----
 * The reference picks its detector by option for every mode (src/decoder.c:863-866) and differentiates in readblock whatever the mode
 * (src/readtape.c:1383-1388,1422).  A handle made for RTFE_WW with find_zeros and / or differentiate runs, through rtfe_ww_detector_scan,
 *   RTFE_WW_ZEROS      find_zeros                   lookfor_zerocrossing                  src/decoder.c:617-649   on the samples
 *   RTFE_WW_DIFFZEROS  find_zeros + differentiate   lookfor_differentiated_zerocrossing   src/decoder.c:654-683   on differentiate()'s output
 *   RTFE_WW_DIFFPEAKS  differentiate                lookfor_peak / refine_peak            src/decoder.c:751-810   on differentiate()'s output
 * (RTFE_WW_PEAKS: neither option - rtfe_ww_scan and rtfe_ww_track above, unchanged.)  Rows, seed_row0, per-track event lists and the state
 * in / state out are as for rtfe_ww_scan; on its seed row and the rows in front of it a track runs NO detector (the `break` of
 * src/decoder.c:861), but differentiate() has run on them (v_last_raw follows every row).  Nothing restarts between blocks, so everything
 * the detectors remember is in the state, rows as ABSOLUTE rows of the tape: a crossing armed in one chunk or attempt - or, after the
 * -deskew rewind, at a row that lies AHEAD - is confirmed correctly in a later one.
 * The ABI version did not move for these entry points: they are additions, nothing that existed changed its layout or its behaviour
 * (rtfe_event, rtfe_ww_track, rtfe_ww_scan and rtfe_ww_initial_state are what they were), and rtfe_create now accepts what it refused. */
enum { RTFE_WW_PEAKS = 0, RTFE_WW_ZEROS = 1, RTFE_WW_DIFFZEROS = 2, RTFE_WW_DIFFPEAKS = 3 };

typedef struct rtfe_ww_dtrack {
   int32_t kind;                    /* RTFE_WW_ZEROS / _DIFFZEROS / _DIFFPEAKS: a blob only meets a handle of its own kind (RTFE_F_STATE_KIND) */
   int32_t delay;                   /* -deskew: this track's delay in samples (0..50), as rtfe_ww_track::delay; differentiate() runs in front of the delay line */
   int32_t v_last_raw;              /* differentiate(): the code (after -invert, so -32768 .. 32768) of the last row read, src/readtape.c:1387 */
   int32_t v_raw_row0;              /* ... and what row 0 of the tape is differentiated against: 0, or after the -deskew rewind the last row the pre-pass read */
   /* the zero-crossing detectors */
   int32_t z_prev, z_top, z_bot;    /* RTFE_WW_ZEROS: v_prev, v_top, v_bot as codes */
   int32_t up_pending, dn_pending;  /* zerocross_up_pending / zerocross_dn_pending */
   float   zf_top, zf_bot;          /* RTFE_WW_DIFFZEROS: v_top, v_bot in volts (differentiated) */
   int32_t have_zero;               /* RTFE_WW_DIFFZEROS: t_firstzero != 0 */
   int64_t row_top, row_bot;        /* RTFE_WW_ZEROS: t_top / t_bot of a pending crossing, as absolute rows */
   int64_t row_firstzero, row_lastzero;   /* RTFE_WW_DIFFZEROS: t_firstzero / t_lastzero as absolute rows */
   /* RTFE_WW_DIFFPEAKS: the window (differentiated volts; a re-seeded window keeps stale slots) and the AGC, as rtfe_ww_track */
   int32_t left, right, countdown, peakcount, heightndx, pad;
   float   maxv, minv;
   float   agc_gain, v_avg_height, v_lasttop, v_lastbot, v_top, v_bot;
   float   heights[10];
   float   ring[64];
} rtfe_ww_dtrack;                    /* 432 bytes */

/* One call of ww_top / ww_bot: an rtfe_event (sample relative to first_row; flags bit 0 = bottom; RTFE_WW_DIFFPEAKS: every field as
 * rtfe_ww_scan fills it, v_peak a differentiated value) and behind it what the 16 bytes cannot hold:
 *   RTFE_WW_ZEROS      back_first = rows from the sign change to the confirming row; the slope gate of src/decoder.c:629,643 is the host's
 *   RTFE_WW_DIFFZEROS  has_zero != 0: back_first / back_last = rows from the first / last exact zero of the run to the confirming row, exact for
 *                      any distance (the run can span an inter-block gap); has_zero = 0: the crossing lies half a sample before the row.
 *                      v_other = the OPPOSITE excursion as the reference still holds it at the callback (it zeroes it only afterwards,
 *                      src/decoder.c:663-667, 676-680): the -deskew pre-pass reads v_top - v_bot (src/decoder.c:484-489)
 * The offsets are signed: after the -deskew rewind a pending row can lie ahead of the row that confirms it. */
typedef struct rtfe_ww_event {
   rtfe_event ev;
   float      v_other;
   uint32_t   has_zero;
   int64_t    back_first, back_last;
} rtfe_ww_event;                     /* 40 bytes */

#define RTFE_F_STATE_KIND 256        /* rtfe_ww_detector_scan: a track's state blob is not of the handle's kind; nothing was scanned */

/* Which detector the handle runs (RTFE_WW_*; -1: not a Whirlwind handle), and the bytes of ONE track's state for it (224 for RTFE_WW_PEAKS).
 * Replaces: the dispatch of src/decoder.c:863-866. */
int    rtfe_ww_state_kind(const rtfe_handle *h);
size_t rtfe_ww_state_bytes(const rtfe_handle *h);
/* The state a tape starts from (host memory, ntrks tracks of rtfe_ww_state_bytes each; state_bytes = the size of the whole buffer, checked).
 * Replaces: init_trackstate, src/decoder.c:425-455. */
int rtfe_ww_detector_initial_state(const rtfe_handle *h, void *tracks, size_t state_bytes);
/* The scan; state_bytes = the size of each of the two state buffers (ntrks rtfe_ww_dtrack).  Errors (rtfe_last_error): a handle of kind
 * RTFE_WW_PEAKS, a state buffer of another size.  A blob of another kind: RTFE_F_STATE_KIND in *d_flags, no events, state handed back as it came.
 * Replaces: lookfor_zerocrossing, lookfor_differentiated_zerocrossing and lookfor_peak behind differentiate() (src/decoder.c:617-683, 751-810;
 * src/readtape.c:1383-1388) for mode WW, at the seam of src/decoder.c:586,604. */
int rtfe_ww_detector_scan(rtfe_handle *h, const int16_t *d_rows, int64_t nrows, int64_t row_base, int64_t first_row, int64_t nscan, int64_t seed_row0,
                          const void *d_state_in, void *d_state_out, size_t state_bytes, uint32_t *d_counts, rtfe_ww_event *d_events,
                          int64_t event_capacity, uint32_t *d_flags, void *stream);

/* ---- CSV text -> int16 rows, on the device ----
 * A logic-analyser export ("time, v0, v1, ..." lines) whose bytes lie in device memory becomes the rows rtfe_scan takes without visiting the host.
 * The numbers are the host loader's (csrc/host/rt_csv.c: the reference's converter, src/csvtbin.c:619-716), bit for bit: its digit-by-digit float
 * scanners, its peak, its quantiser and its clip count.  Handle-free and queued on `stream`; every pointer is device memory unless said otherwise.
 * The ABI version did not move: additions only, and rtfe_kernel_count() stays what it was (these kernels are no spans of a scan).
 * A WINDOW is a contiguous piece of the file's bytes: d_text 16-byte aligned and readable up to nbytes rounded up to 16, nbytes < 2^32.
 *
 * rtfe_csv_index: the lines of a window.  d_starts[i], i < lines: the offset of line i's first byte; d_starts[lines] == consumed, the offset behind the
 *   last complete line (the next window starts there), so line i is [d_starts[i], d_starts[i + 1]), its '\n' included.  is_last: the window ends the
 *   file, and the bytes behind its last '\n', if there are any, are a line too (fgets returns an unterminated last line, and nothing for an empty one).
 *   longest: the longest line, '\n' included (at most 2^31 - 1 is reported).  d_starts holds starts_cap + 1 entries: a window with more lines than
 *   starts_cap sets RTFE_CSV_STARTS_FULL, writes the entries that fit and nothing out of bounds - lines, consumed and longest are right all the same:
 *   come back with lines entries.  d_scratch: rtfe_csv_index_scratch_bytes(nbytes), 16-byte aligned.
 * rtfe_csv_peak: lines [first_line, first_line + nlines) of an indexed window - the time field skipped, then ntrks fields: *d_peak = max(*d_peak,
 *   |field * scale|) (the caller starts it at 0; exact and independent of order).  rt_csv_survey's peak.
 * rtfe_csv_parse: nkept lines first_line, first_line + step, ... of an indexed window -> d_rows[j * ntrks + (perm ? perm[k] : k)] = the code of line j's
 *   field k (missing fields are 0); perm is HOST memory and may be NULL.  *d_clipped += the codes that met a rail (+-32767 included, as on the host).
 *   ntrks outside 1 .. 19: -3, a perm entry outside 0 .. ntrks - 1: -4 (rt_csv_load's codes; rtfe_last_error says which). rt_csv_load's rows.
 * rtfe_csv_graph: the converter's -graph and the peak its -redo needs (src/csvtbin.c:704-706, 719-722, 732).  The kept lines are rtfe_csv_parse's
 *   (first_line, step, nkept); kept line j is sample first_sample + j of the pass (0-based), and for bins below nbins
 *   d_bins[(first_sample + j) / graphbin] = max(its old value, max_k |field_k * scale| of the line); *d_peak (may be NULL) = max(*d_peak, the same over all
 *   lines).  Non-negative floats compared as their bit patterns: exact and independent of order, so calls for different windows of a file may meet in one
 *   bin.  The caller zeroes both; nothing is written at or behind d_bins + nbins (nbins 0: d_bins may be NULL).  Refusals: rtfe_csv_parse's, and -34 for
 *   graphbin < 1, nbins < 0, first_sample < 0.  The sign flip of -invert does not change a magnitude, and -order= only moves columns: neither is an argument. */
#define RTFE_CSV_STARTS_FULL 1
typedef struct rtfe_csv_window { int64_t lines; int64_t consumed; uint32_t longest; uint32_t flags; } rtfe_csv_window;      /* 24 bytes */
size_t rtfe_csv_index_scratch_bytes(uint64_t nbytes);
int rtfe_csv_index(const void *d_text, uint64_t nbytes, int is_last, uint32_t *d_starts, int64_t starts_cap, void *d_scratch, size_t scratch_bytes,
                   rtfe_csv_window *d_out, void *stream);
int rtfe_csv_peak(const void *d_text, const uint32_t *d_starts, int64_t first_line, int64_t nlines, int ntrks, float scale, float *d_peak, void *stream);
int rtfe_csv_parse(const void *d_text, const uint32_t *d_starts, int64_t first_line, int64_t step, int64_t nkept, int ntrks, const int *perm, int invert,
                   float scale, float maxvolts, int16_t *d_rows, int64_t *d_clipped, void *stream);
int rtfe_csv_graph(const void *d_text, const uint32_t *d_starts, int64_t first_line, int64_t step, int64_t nkept, int ntrks, float scale,
                   int64_t first_sample, int64_t graphbin, float *d_bins, int64_t nbins, float *d_peak, void *stream);

/* ---- int16 rows -> CSV text, on the device: the converter's -read (src/csvtbin.c:570-595) ----
 * The mirror image of the block above: rows that are resident in device memory become the text the reference's `csvtbin -read` prints for them, byte for
 * byte - "%12.8f, " of (double)t_ns / 1e9, then per column "%9.5f, " of the float32 value code / 32767 * maxvolts (negated if invert, plus k * stagger summed
 * in float32), then '\n'; the last field keeps its ", ".  The two title lines are the caller's (csrc/host/rt_csvout.c writes them).  The host writer
 * rt_csv_export_write (csrc/host/rt_csv.h) prints the same lines with fprintf; the kernels (csrc/rtfe_csvout.hip) make both fields in exact integer
 * arithmetic.  Handle-free and queued on `stream`; every pointer is device memory unless said otherwise.  The ABI version did not move: additions only, and
 * rtfe_kernel_count() stays what it was (these kernels are no spans of a scan).
 * A WINDOW is rows [first_row, first_row + nrows) of the tape d_rows[.][ntrks] (d_rows points at row 0: a row's time is tstart_ns + row * tdelta_ns); its text
 * is one contiguous piece at d_text (16-byte aligned, text_cap bytes), line after line from offset 0.
 *
 * rtfe_csv_format: the window's text.  *d_out: bytes = the length of the whole text, rows = nrows, longest = its longest line ('\n' included).  A text
 *   longer than text_cap sets RTFE_CSV_TEXT_FULL: the first text_cap bytes are written, nothing at or behind d_text + text_cap, and bytes is right all the
 *   same - come back with that much.  rtfe_csv_format_max_bytes(nrows, ntrks) always suffices.  d_scratch: rtfe_csv_format_scratch_bytes(nrows), 16-byte aligned.
 *   a->perm is HOST memory and may be NULL: column k prints d_rows[.][perm[k]].
 *   Two layouts, chosen here (rtfe_csv_format_path says which: 1 / 0, or the refusal): UNIFORM where every line provably has 14 + 11 ntrks + 1 bytes - the
 *   window's last time below 1000 s and |maxvolts| 32768 / 32767 + (ntrks - 1) |stagger| below 99 -, one kernel; GENERAL otherwise, a length pass and a prefix
 *   sum in front of it.
 *   Refusals: ntrks outside 1 .. 19: -3; a perm entry outside 0 .. ntrks - 1: -4; d_text not 16-byte aligned: -31; scratch too small: -32; a negative row
 *   range or more rows than a launch takes: -34; |maxvolts| 32768 / 32767 + (ntrks - 1) |stagger| not finite or not below 2^20 (the integer formatter's
 *   domain): -46; the window's last time 2^49 ns (6.5 days) or more (the time field's proof): -47.  rtfe_last_error says which. */
#define RTFE_CSV_TEXT_FULL 1
typedef struct rtfe_csv_format_args {
   int ntrks; int invert; float maxvolts; float stagger; uint64_t tstart_ns; uint32_t tdelta_ns;
   const int *perm;                  /* host, may be NULL: column k prints rows[.][perm[k]] */
} rtfe_csv_format_args;
typedef struct rtfe_csv_text { uint64_t bytes; int64_t rows; uint32_t flags; uint32_t longest; } rtfe_csv_text;      /* 24 bytes */
size_t rtfe_csv_format_max_bytes(int64_t nrows, int ntrks);       /* worst-case text of a window: 17 + 16 ntrks + 1 bytes a line */
size_t rtfe_csv_format_scratch_bytes(int64_t nrows);
int    rtfe_csv_format_path(int64_t first_row, int64_t nrows, const rtfe_csv_format_args *a);
int    rtfe_csv_format(const int16_t *d_rows, int64_t first_row, int64_t nrows, const rtfe_csv_format_args *a,
                       void *d_text, size_t text_cap, void *d_scratch, size_t scratch_bytes, rtfe_csv_text *d_out, void *stream);

/* ---- the interpreted text dump of a SIMH .tap image (the reference's -tapread, src/textfile.c and src/tapread.c), made on the device.  Handle-free.
 * The image's bytes lie in device memory; its items - records, tape marks, the reader's messages, in file order - come from the host's reader (rt_tap_items,
 * csrc/host/rt_textfile.h; the same 16 bytes an item) and are given twice: items on the host, where they are checked against image_bytes and counted, and
 * d_items, the same table on the device, which the kernels read.  A window of a large image is a slice of the table.
 * rtfe_text_format writes the BODY of the terse layout - per record the "%c%4d: " prefix ('!' in front of a record whose marker has the error bit), its lines
 * of numbers and / or characters with seven blanks in front of every further line, "tape mark", the messages - byte for byte what the host writer
 * (rt_text_record ...) puts between the three title lines and the trailer, which stay the host's.  Options as the reference's: numtype 0 none / 1 hex / 2 octal /
 * 3 octal2, chartype 0 none / 1 BCD / 2 EBCDIC / 3 ASCII / 4 B5500 / 5 sixbit / 6 SDS / 7 SDSM / 8 flexo / 9 adage / 10 adagetape / 11 CDC / 12 Univac,
 * linesize 4..400 (0: 32 with both types, otherwise 64), dataspace 0..400 (-1: 2 under octal2, otherwise 0), linefeed, ntrks (up to 7: two octal digits a byte).
 * Refused with an error string: verbose != 0 (the decode path's layout: its block lines are host strings) and neither a number nor a character type (the list
 * of block sizes is sequential and trivial: the host writes it).
 * nlinefeeds: with linefeed, at least the number of 0x0a bytes in the items' data (the whole slice of the image may be counted); it sizes the scratch, and a
 *   count that is too small sets RTFE_TEXT_SCRATCH_FULL: no text is written.  Ignored without linefeed.
 * *d_out: bytes = the length of the whole body, lines, stretches (pieces of records between the linefeeds that break lines; without linefeed: the items).  A
 *   body longer than text_cap sets RTFE_TEXT_FULL: the first text_cap bytes are written, nothing at or behind d_text + text_cap, and bytes is right all the
 *   same.  rtfe_text_format_max_bytes always suffices (exact without linefeed unless ntrks <= 7 prints octal).  d_text 16-byte, d_scratch 8-byte aligned. */
#define RTFE_TEXT_FULL 1
#define RTFE_TEXT_SCRATCH_FULL 2
typedef struct rtfe_text_options { int numtype, chartype, linesize, dataspace, linefeed, ntrks, verbose; } rtfe_text_options;
typedef struct rtfe_text_item { uint64_t offset; uint32_t length; uint16_t kind, flag; } rtfe_text_item;      /* kind 0 record / 1 tape mark / 2 message (flag: which) */
typedef struct rtfe_text_out { uint64_t bytes, lines, stretches; uint32_t flags, reserved; } rtfe_text_out;      /* 32 bytes */
size_t rtfe_text_format_max_bytes(const rtfe_text_item *items, int64_t nitems, uint64_t nlinefeeds, const rtfe_text_options *o);        /* 0: refused */
size_t rtfe_text_format_scratch_bytes(const rtfe_text_item *items, int64_t nitems, uint64_t nlinefeeds, const rtfe_text_options *o);
int    rtfe_text_format(const void *d_image, uint64_t image_bytes, const rtfe_text_item *items, const rtfe_text_item *d_items, int64_t nitems, uint64_t nlinefeeds,
                        const rtfe_text_options *o, void *d_text, size_t text_cap, void *d_scratch, size_t scratch_bytes, rtfe_text_out *d_out, void *stream);

/* ---- the tape writer: flux transitions -> the int16 rows a head would have read, rendered on the device.  Handle-free.
 * The other direction of everything above.  The host encoder (rt_tapewrite_encode / rt_tapewrite_raw, csrc/host/rt_tapewrite.h) turns a SIMH .tap image into
 * a SLOT STREAM and a BLOCK TABLE; rtfe_tape_render turns a window of the tape they describe into rows, byte for byte what the host renderer
 * rt_tapewrite_render gives.  Queued on `stream`, no allocation, no host synchronisation.  The ABI version did not move: additions only, and
 * rtfe_kernel_count() stays what it was (this kernel is no span of a scan).
 *
 * The model (csrc/host/rt_tapewrite_model.h holds it as code, shared by the host renderer and the kernel):
 *   A slot is a place where flux may change: bit t of `flux` = track t has a transition there, bit t of `neg` = that transition reads as a negative pulse.
 *   Slot s of a block lies at cell position s * pitch, pitch = 1 (pitch_shift 0: NRZI, GCR) or 1/2 cell (pitch_shift 1: PE).  A block of the table owns
 *   rows [first_row, first_row + rows) of the tape and slots [first_slot, first_slot + nslots) of the stream; blocks are sorted and do not overlap; rows
 *   that belong to no block are gap.  With r the row counted from the block's first, a transition of track t in slot s has
 *      c = (8 + s * pitch + 0.5 + skew[t] + jit) * spb,   jit = g(jkey[t], first_slot + s) * jitter          (0 where jitter == 0)
 *   and adds  a * (1 / (1 + d * d) - edge),  d = (r - c) / w,  a = +-amp[t], to every row of ITS OWN block with |r - rint(c)| <= K.  A sample is the sum of
 *   these from 0.0 in ascending slot order, plus g(nkey[t], row of the tape) * noise_mv * 1e-3 (where noise_mv > 0, in gaps too), quantised
 *   rint(v / maxvolts * 32767) and clipped to +-32767.  Every operation is an IEEE double + - * / or rint in the order written, no FMA, no libm.
 *   g(key, n): z = key + n * 0x9E3779B97F4A7C15, the splitmix64 finaliser over z, its four 16-bit fields summed (Irwin-Hall), minus 131070, times
 *   0x1.bb67ae86627e8p-16 (one over the sum's standard deviation): mean 0, variance 1, close to normal, and BOUNDED: |g| <= 3.4641.  A function of the
 *   absolute row / slot, so a window of a tape is the same slice of the whole.  rt_tapewrite_params fills the structure from a physical description.
 *
 * rtfe_tape_render: rows [first_row, first_row + nrows) of the tape into d_rows[0 .. nrows * ntrks).  `blocks` (host) and d_blocks (device) are the same
 *   table; the host copy is checked, the kernel reads the device copy.  d_slots: the whole stream, device.  p: host.
 * Memory contract: reads d_slots[0 .. nslots) and d_blocks[0 .. nblocks); writes exactly the bytes of d_rows[0 .. nrows * ntrks) - none in front, none
 *   behind: a workgroup takes a span of rtfe_tape_render_span_rows(ntrks) rows ON THE TAPE'S OWN GRID (row 0 of the tape starts a span, whatever the
 *   window), stages its samples in LDS and stores whole aligned 16-byte vectors; the partial vectors at a span's ends - at the window's two ends, and where
 *   a span's bytes are no multiple of 16 - are stored sample by sample.
 * Refusals, all before anything is queued (d_rows is left alone): a null pointer (d_slots and the block tables may be null when their count is 0): -1;
 *   p->ntrks outside 1 .. 19: -3; d_rows not 16-byte aligned: -31; a negative count or row, or more rows than a launch takes: -34; a parameter that is
 *   no finite number where the model needs one, maxvolts or spb or w not above 0, pitch_shift outside 0 .. 1: -62; a block table that is not sorted, overlaps,
 *   has a negative field, names slots outside [0, nslots) or more than 2^31 - 1 slots in a block: -61; a reach K outside 0 .. RTFE_TAPE_MAX_REACH, or a
 *   slot pitch so fine (spb * pitch rows a slot) that the slots one span needs - (span rows + 2 * (K + 2 + ceil((max |skew| + 3.4641 jitter) * spb))) /
 *   (spb * pitch) + 7 - exceed the RTFE_TAPE_MAX_SLOTS the kernel stages: -60.  rtfe_last_error says which. */
#define RTFE_TAPE_MAX_REACH 2048
#define RTFE_TAPE_MAX_SLOTS 2048
typedef struct rtfe_tape_slot { uint32_t flux, neg; } rtfe_tape_slot;                                    /* 8 bytes */
typedef struct rtfe_tape_block { int64_t first_row, rows, first_slot, nslots; } rtfe_tape_block;        /* 32 bytes */
typedef struct rtfe_tape_params {
   int32_t ntrks, pitch_shift, K, reserved;
   double spb, w, edge, maxvolts, noise_mv, jitter;      /* rows a cell; the pulse's half width in rows; 1 / (1 + (K / w)^2); ...; sigma in cells */
   double amp[19], skew[19];                              /* volts; cells */
   uint64_t nkey[19], jkey[19];                           /* the generator's keys: noise by row, jitter by slot */
} rtfe_tape_params;
int64_t rtfe_tape_render_span_rows(int ntrks);                  /* rows one workgroup takes: for tests and tools that aim at its seams */
int rtfe_tape_render(const rtfe_tape_slot *d_slots, int64_t nslots, const rtfe_tape_block *blocks, const rtfe_tape_block *d_blocks, int64_t nblocks,
                     const rtfe_tape_params *p, int64_t first_row, int64_t nrows, int16_t *d_rows, void *stream);

#ifdef __cplusplus
}
#endif
#endif
