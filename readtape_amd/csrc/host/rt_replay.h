/* rt_replay.h — event replay: device front-end output -> host block decoders -> SIMH .tap (see rt_replay.c) */
#ifndef RT_REPLAY_H
#define RT_REPLAY_H
#include "rt_decode.h"
#include "rt_frontend.h"
#include "rt_textfile.h"

#ifdef __cplusplus
extern "C" {
#endif

/* asks the caller for an exact device scan (rtfe_scan_exact) of one attempt: rows [reset_row, end_row) of the
 * scanned slice, one parameter set.  On success fills *burst, counts[ntrks], *events (regions of *cap events per
 * track, track-major) and returns 0. */
typedef int  (*rt_exact_fn)(void *user, int64_t reset_row, int64_t end_row, int parmset,
                            rtfe_burst *burst, uint32_t *counts, rtfe_event **events, uint32_t *cap);
typedef void (*rt_exact_free_fn)(void *user, rtfe_event *events);

/* Whirlwind: the device's detector keeps its state across attempts, so the replay fetches its events in chunks of rows, handing the
 * state in and getting it back (include/rt_frontend.h: rtfe_ww_scan; with -zeros / -differentiate rtfe_ww_detector_scan).  first_row / nscan /
 * seed_row0 as there; state blobs are opaque here, ntrks tracks of the size the front end reports (host memory); events: [ntrks][cap] records
 * (sample relative to first_row) - rtfe_event for the peak detector, rtfe_ww_event for the other three -, counts[ntrks].  Returns 0, or the
 * RTFE_F_* flags of a scan that could not be delivered. */
typedef int (*rt_ww_scan_fn)(void *user, int64_t first_row, int64_t nscan, int64_t seed_row0, const void *state_in, void *state_out,
                             uint32_t *counts, rtfe_event *events, uint32_t cap);

struct rt_replay {
   struct rt_dec *d;
   int     ntrks, nparm;
   int     W[RT_MAXPARMSETS];          /* rtfe_pkww_width() per parameter set */
   int64_t nrows, row_base, tstart_ns, tdelta_ns;
   const rtfe_burst *bursts; int64_t nbursts;
   const uint32_t   *counts;
   const rtfe_event *events;
   rt_exact_fn exact; rt_exact_free_fn exact_free; void *exact_user;
   int64_t pos, saved_pos, cur_row; double saved_time;
   int64_t stop_row;                   /* fragment decode: no attempt starts at or behind this row */
   int     end_counted;                /* ... a first attempt found the end: lines_in has its + 1 */
   /* Whirlwind */
   rt_ww_scan_fn ww_scan; void *ww_user;
   unsigned char *ww_state, *ww_chunk_state, *ww_chunk_end;   /* ntrks tracks of ww_track_bytes each: at the attempt's start / at the chunk's first row / behind the chunk */
   size_t  ww_track_bytes, ww_event_bytes;
   rtfe_event *ww_events; uint32_t *ww_counts; uint32_t ww_cap; int64_t ww_chunk_rows;
   int     find_zeros;                 /* events are confirmed zero crossings: the slope gate is applied here */
   FILE   *evtf;                       /* optional dump of every delivered transition (oracle/ref_event_shim.c record format) */
   /* statistics */
   int64_t attempts, exact_scans, chained, events_delivered, agc_mismatches;
   int64_t device_failures;            /* attempts the device could not deliver (exact scan refused / overflowed): the decode stops there */
   int64_t reference_fatal, fatal_row, fatal_trk;   /* an RTFE_EV_FATAL marker was reached: the reference exits there (src/decoder.c:782) */
};

int  rt_replay_readblock(void *ctx, int retry);
void rt_replay_save_pos(void *ctx);
void rt_replay_restore_pos(void *ctx);

struct rt_replay_stats {
   int64_t attempts, exact_scans, chained, events_delivered, agc_mismatches;
   int32_t blocks, tapemarks, blocks_with_errors, blocks_with_warnings, blocks_unusable, all_ok;
   int64_t data_bytes;
   int64_t device_failures;            /* > 0: the decode stopped early because the device could not deliver an attempt */
   int64_t reference_fatal, fatal_row, fatal_trk;   /* != 0: the decode stopped where the reference's "AGC gain bad" assert ends its run */
};

/* Decodes a whole scanned tape: builds a decoder for `opt` (+ `parmsets`, NULL = built-in sets), replays the
 * device output through the retry/selection driver and writes tap_path / log_path (NULL = none). */
int rt_replay_run(const struct rt_options *opt, const struct rt_parms *parmsets, int nparm,
                  int64_t tdelta_ns, int64_t tstart_ns, int64_t nrows, int64_t row_base, const int *W,
                  const rtfe_burst *bursts, int64_t nbursts, const uint32_t *counts, const rtfe_event *events,
                  rt_exact_fn exact, rt_exact_free_fn exact_free, void *user,
                  const char *tap_path, const char *log_path, const char *evt_path, struct rt_replay_stats *stats);


/* -deskew (src/readtape.c:1675-1717): the pre-pass over a scan made WITHOUT deskew delays -> delays[ntrks] in samples,
 * *nblks = blocks used (-1: a track without transitions), *hit_end = the scan ended before the stopping rule was met.
 * The decode of the re-scanned tape then continues the same log / event-dump files (rt_replay_run_after_deskew);
 * append != 0: the pre-pass itself continues files a density detection started. */
int rt_replay_deskew(const struct rt_options *opt, const struct rt_parms *parmsets, int nparm,
                  int64_t tdelta_ns, int64_t tstart_ns, int64_t nrows, int64_t row_base, const int *W,
                  const rtfe_burst *bursts, int64_t nbursts, const uint32_t *counts, const rtfe_event *events,
                  rt_exact_fn exact, rt_exact_free_fn exact_free, void *user,
                  const char *log_path, const char *evt_path, int append, int *delays, int *nblks, int *hit_end);
/* density detection (src/readtape.c:1656-1672) over a scan made with bpi = 0 (window of 8, no AGC feedback):
 * *bpi = the standard density chosen (0: the implied density *implied is not close to one), *nblks, *hit_end as above. */
int rt_replay_density(const struct rt_options *opt, const struct rt_parms *parmsets, int nparm,
                  int64_t tdelta_ns, int64_t tstart_ns, int64_t nrows, int64_t row_base, const int *W,
                  const rtfe_burst *bursts, int64_t nbursts, const uint32_t *counts, const rtfe_event *events,
                  rt_exact_fn exact, rt_exact_free_fn exact_free, void *user,
                  const char *log_path, const char *evt_path, float *bpi, float *implied, int *nblks, int *hit_end);
int rt_replay_run_fragment(const struct rt_options *opt, const struct rt_parms *parmsets, int nparm,
                  int64_t tdelta_ns, int64_t tstart_ns, int64_t nrows, int64_t row_base, const int *W,
                  const rtfe_burst *bursts, int64_t nbursts, const uint32_t *counts, const rtfe_event *events,
                  rt_exact_fn exact, rt_exact_free_fn exact_free, void *user,
                  const char *tap_path, const char *log_path, const char *evt_path, struct rt_replay_stats *stats,
                  int64_t start_row, int64_t stop_row);
/* The same for nfrag fragments of one scan side by side, a thread each (the streaming reader's sub-fragments of a window: cut at burst
 * boundaries, each with its own decoder context and its own piece of the .tap).  stats[nfrag], seconds[nfrag] (each fragment's own time).
 * Returns 0, or the first failing fragment's code. */
int rt_replay_run_fragments(const struct rt_options *opt, const struct rt_parms *parmsets, int nparm,
                  int64_t tdelta_ns, int64_t tstart_ns, int64_t nrows, int64_t row_base, const int *W,
                  const rtfe_burst *bursts, int64_t nbursts, const uint32_t *counts, const rtfe_event *events,
                  rt_exact_fn exact, rt_exact_free_fn exact_free, void *user,
                  int nfrag, const char *const *tap_paths, const int64_t *start_rows, const int64_t *stop_rows, struct rt_replay_stats *stats, double *seconds);
/* The reader's positional read of nbytes at file offset `off` into dst, as nthreads pieces side by side (from the page cache one thread copies
 * ~13 GB/s).  Returns 0, -1 on a short read or an error. */
int rt_read_mt(int fd, void *dst, int64_t off, int64_t nbytes, int nthreads);
int rt_replay_run_ww(const struct rt_options *opt, const struct rt_parms *parmsets,
                  int64_t tdelta_ns, int64_t tstart_ns, int64_t nrows, int W0, rt_ww_scan_fn scan, void *user, const void *initial_state, int64_t chunk_rows,
                  const char *tap_path, const char *out_base, const char *in_name, const char *log_path, const char *evt_path, struct rt_replay_stats *stats,
                  int deskew, int *delays_out);
/* ... with the detector the options name (opt->find_zeros / do_differentiate; neither: exactly rt_replay_run_ww): track_bytes = the size of one
 * track's state as the front end reports it (rtfe_ww_state_bytes); -4 if that is not the size of the detector's state. */
int rt_replay_run_ww_detector(const struct rt_options *opt, const struct rt_parms *parmsets,
                  int64_t tdelta_ns, int64_t tstart_ns, int64_t nrows, int W0, rt_ww_scan_fn scan, void *user, const void *initial_state, size_t track_bytes,
                  int64_t chunk_rows, const char *tap_path, const char *out_base, const char *in_name, const char *log_path, const char *evt_path,
                  struct rt_replay_stats *stats, int deskew, int *delays_out);
int rt_replay_run_named(const struct rt_options *opt, const struct rt_parms *parmsets, int nparm,
                  int64_t tdelta_ns, int64_t tstart_ns, int64_t nrows, int64_t row_base, const int *W,
                  const rtfe_burst *bursts, int64_t nbursts, const uint32_t *counts, const rtfe_event *events,
                  rt_exact_fn exact, rt_exact_free_fn exact_free, void *user,
                  const char *out_base, const char *in_name, const char *log_path, const char *evt_path, int append, struct rt_replay_stats *stats);
int rt_replay_run_after_deskew(const struct rt_options *opt, const struct rt_parms *parmsets, int nparm,
                  int64_t tdelta_ns, int64_t tstart_ns, int64_t nrows, int64_t row_base, const int *W,
                  const rtfe_burst *bursts, int64_t nbursts, const uint32_t *counts, const rtfe_event *events,
                  rt_exact_fn exact, rt_exact_free_fn exact_free, void *user,
                  const char *tap_path, const char *log_path, const char *evt_path, struct rt_replay_stats *stats);
/* -textfile: the next decode this thread starts (rt_replay_run, _run_named, _run_after_deskew, _run_ww, _run_ww_detector) writes the interpreted text
 * file of <base> in the verbose layout beside its .tap; o->ntrks is taken from the decode.  o == NULL takes the request back. */
void rt_replay_set_text(const rt_text_options *o, const char *base, const char *created);
/* --peakstats: the next decode this thread starts (rt_replay_run, _run_named, _run_after_deskew, _run_ww, _run_ww_detector, with the rt_replay_deskew
 * pre-pass in front of it) gathers the reference's flux-transition statistics in its main pass too, writes <base>.peakstats.csv - and a pre-pass
 * <base>.peakstats_deskew.csv - and logs the head-skew verdict under the summary.  quiet: the reference's -q (only the _deskew file, no log lines);
 * deskew: its `deskew` flag (-deskew or -skew= was given: picks the sentence).  base == NULL takes the request back and forgets the results.
 * rt_replay_get_peakstats(which: 0 the decode's, 1 the pre-pass'): the histogram behind the file (counts[RT_MAXTRKS][RT_PEAKSTAT_BUCKETS],
 * trksums[RT_MAXTRKS]) and skew_compute_deskew's answer, of the last such decode on this thread; 0 if there is none. */
void rt_replay_set_peakstats(const char *base, int quiet, int deskew);
int  rt_replay_get_peakstats(int which, float *leftbin, float *binwidth, int32_t *counts, int32_t *trksums, int *ok, float *peak_frac, float *stddev_frac);

/* ---- the windowed decode: fragments journal their blocks, ONE finisher puts them out ----
 * A journal holds what a fragment's replay would have put out - per block the type, the data words, the chosen attempt's results, tries and parameter
 * set, the times, the row behind it, and the running counters of the summary - in memory, in a private format.  rt_replay_journal_fragments is
 * rt_replay_run_fragments in journal mode: journals[i] takes fragment i's blocks, nothing is written.
 * Peak statistics: journals made with an rt_peakbins record into their own histogram on the bins the tape's first transition fixes; `first` marks the tape's
 * first fragment, which publishes them; a fragment that does not know them yet keeps its transitions for the finisher (nobody waits, so any order and
 * any number of threads will do).  snapshots: every record carries the histogram so far (wanted with a block limit: the finisher stops inside a journal). */
struct rt_journal;
struct rt_peakbins;
struct rt_finisher;
struct rt_peakbins *rt_peakbins_new(void);
void rt_peakbins_free(struct rt_peakbins *b);
struct rt_journal *rt_journal_new(struct rt_peakbins *bins, int first, int snapshots);
void    rt_journal_free(struct rt_journal *j);
int64_t rt_journal_bytes(const struct rt_journal *j);
int     rt_journal_records(const struct rt_journal *j);
int     rt_journal_stats(const struct rt_journal *j, struct rt_replay_stats *stats);      /* the fragment's own replay statistics (-1: not run) */
int64_t rt_journal_final_row(const struct rt_journal *j);      /* the absolute row at which the fragment's last attempt ended (-1: not run) */
/* one block of a context into a journal, as the fragment replay does it (blktype: RT_BS_TAPEMARK, _BLOCK or _BADBLOCK; d->parmset names the results) */
void    rt_journal_record(struct rt_journal *j, struct rt_dec *d, int blktype);
void    rt_journal_close(struct rt_journal *j);                /* ... and the end of such a journal: it is whole */
int rt_replay_journal_fragments(const struct rt_options *opt, const struct rt_parms *parmsets, int nparm,
                  int64_t tdelta_ns, int64_t tstart_ns, int64_t nrows, int64_t row_base, const int *W,
                  const rtfe_burst *bursts, int64_t nbursts, const uint32_t *counts, const rtfe_event *events,
                  rt_exact_fn exact, rt_exact_free_fn exact_free, void *user,
                  int nfrag, struct rt_journal *const *journals, const int64_t *start_rows, const int64_t *stop_rows, double *seconds);
/* The finisher is one decoder context around the output stage of the resident decode: it takes the calling thread's requests (rt_replay_set_text,
 * rt_driver_set_run, and with `bins` rt_replay_set_peakstats), names its files as rt_replay_run_named (out_base) or rt_replay_run (tap_path) does, and
 * appends to the log a pre-pass began (append).  rt_journal_finish: the next fragment's journal, in tape order, whole fragments only (0; 1: the block
 * limit is reached, nothing more is wanted; -1: not a finished journal).  rt_journal_finisher_end: the end of the files, the summary (with in_name), the
 * statistics' report; *stats as a resident replay's, *seconds the finisher's own time; the finisher is gone.  One thread makes all these calls. */
struct rt_finisher *rt_journal_finisher_new(const struct rt_options *opt, const struct rt_parms *parmsets, int nparm, int64_t tdelta_ns,
                  const char *tap_path, const char *out_base, const char *in_name, const char *log_path, int append, struct rt_peakbins *bins);
int rt_journal_finish(struct rt_finisher *f, struct rt_journal *j);
int rt_journal_finisher_end(struct rt_finisher *f, struct rt_replay_stats *stats, double *seconds);

#ifdef __cplusplus
}
#endif
#endif
