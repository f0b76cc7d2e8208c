/* rt_replay.c — drives the host block decoders from the device front end's event lists.
 *
 * This is the counterpart of the reference's readblock()/process_sample() control flow
 * (src/readtape.c:1396-1517, src/decoder.c:817-905) with the per-sample detectors removed: the
 * detectors ran on the GPU (include/rt_frontend.h) and left, per block attempt and parameter set, the
 * exact sequence of top/bottom detections.  What remains sequential — and is reproduced here row for
 * row, but only at rows where something happens — is:
 *   - the staggered track start (t_lastpeak = time of row s0+trk, src/decoder.c:855-861),
 *   - the NRZI mid-bit timer (src/decoder.c:844-845), the PE and GCR idle timers (:868-888),
 *   - the interblock skip (src/decoder.c:841-842, 901-904),
 *   - end of data (src/readtape.c:1410-1413),
 * in exactly the order process_sample() interleaves them with the detections of a row.
 *
 * Speculation check: an attempt that starts at row s0 may use burst b only if
 * zone_first <= s0 <= safe_last and the burst is not flagged; it may run past the burst's end only
 * while it has not seen a single event (fresh state == the next burst's fresh state).  Otherwise the
 * `exact` callback is asked for an exact device scan of this one attempt.  No detector code runs here.
 */
#include "rt_replay.h"

#include <math.h>
#include <pthread.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

static double time_of_row(const struct rt_replay *rp, int64_t row) {        /* src/readtape.c:1423 */
   return (double)(rp->tstart_ns + row * rp->tdelta_ns) / 1e9; }

/* smallest row >= from with pred(time_of_row(row)) true, for a predicate that is monotone in time;
 * `guess_time` is where it is expected to flip.  Returns limit if not before limit. */
typedef int (*time_pred)(const struct rt_dec *d, const struct rt_trk *t, double timenow);
static int64_t first_row_where(const struct rt_replay *rp, time_pred pred, const struct rt_trk *t,
                               double guess_time, int64_t from, int64_t limit) {
   double g = (guess_time * 1e9 - (double)rp->tstart_ns) / (double)rp->tdelta_ns;
   int64_t r = (g < (double)from) ? from : (g > (double)limit ? limit : (int64_t)g);
   if (r < from) r = from;
   if (r > limit) r = limit;
   struct rt_dec *d = rp->d;
   /* walk down while the predicate still holds just below, then up until it holds */
   while (r > from && pred(d, t, time_of_row(rp, r - 1))) --r;
   while (r < limit && !pred(d, t, time_of_row(rp, r))) ++r;
   return r; }

static int pred_nrzi(const struct rt_dec *d, const struct rt_trk *t, double timenow) {
   (void)t;
   return timenow > d->nrzi.t_lastclock + 2 * d->nrzi.clkavg.t_bitspaceavg; }     /* src/decoder.c:844 */
static int pred_pe(const struct rt_dec *d, const struct rt_trk *t, double timenow) {
   (void)d;
   return timenow - t->t_lastpeak > t->clkavg.t_bitspaceavg * 2.5f; }            /* src/decoder.c:868 */
static int pred_gcr(const struct rt_dec *d, const struct rt_trk *t, double timenow) {
   (void)d;
   return timenow > t->t_lastpeak + 6.00 * t->clkavg.t_bitspaceavg; }            /* src/decoder.c:880 */

/* ---- the event source of one attempt: per-track lists of one (burst, parmset) ---- */
struct evsrc {
   const unsigned char *list[RT_MAXTRKS];
   size_t stride;           /* bytes from one record of a list to the next: sizeof(rtfe_event), or sizeof(rtfe_ww_event) (an rtfe_event in front) */
   uint32_t n[RT_MAXTRKS], at[RT_MAXTRKS];
   int64_t nr[RT_MAXTRKS];  /* absolute row of each track's next event, INT64_MAX when its list is used up (evsrc_sync keeps it) */
   int64_t reset;           /* absolute row of sample 0 */
   int64_t end;             /* rows >= end are not covered by this source */
};

static inline const rtfe_event *evsrc_ev(const struct evsrc *s, int t, uint32_t i) {
   return (const rtfe_event *)(s->list[t] + (size_t)i * s->stride); }

static inline void evsrc_sync(struct evsrc *s, int t) {
   s->nr[t] = s->at[t] < s->n[t] ? s->reset + (int64_t)evsrc_ev(s, t, s->at[t])->sample : INT64_MAX; }

static void evsrc_from_burst(struct evsrc *s, const struct rt_replay *rp, int64_t b, int parmset) {
   const rtfe_burst *B = &rp->bursts[b];
   if (rp->find_zeros) parmset = 0;           /* the zero-crossing front end does not depend on the parameter set */
   s->stride = sizeof(rtfe_event);
   for (int t = 0; t < rp->ntrks; ++t) {
      s->list[t] = (const unsigned char *)(rp->events + B->event_base + (uint64_t)(parmset * rp->ntrks + t) * B->event_cap);
      s->n[t] = rp->counts[((size_t)b * rp->nparm + parmset) * rp->ntrks + t];
      s->at[t] = 0; }
   s->reset = B->reset_sample - rp->row_base;
   s->end = B->end_sample - rp->row_base;
   for (int t = 0; t < rp->ntrks; ++t) evsrc_sync(s, t); }

static inline int64_t evsrc_next_row(const struct evsrc *s, int ntrks) {
   int64_t best = INT64_MAX;
   for (int t = 0; t < ntrks; ++t) if (s->nr[t] < best) best = s->nr[t];
   return best; }

static void evsrc_skip_before(struct evsrc *s, int ntrks, int64_t row) {
   for (int t = 0; t < ntrks; ++t)
      if (s->nr[t] < row) {
         while (s->at[t] < s->n[t] && s->reset + evsrc_ev(s, t, s->at[t])->sample < row) ++s->at[t];
         evsrc_sync(s, t); } }

static int64_t find_burst(const struct rt_replay *rp, int64_t s0) {
   /* last burst whose zone starts at or before s0 */
   int64_t lo = 0, hi = rp->nbursts - 1, ans = -1;
   const int64_t a = s0 + rp->row_base;
   while (lo <= hi) {
      int64_t mid = (lo + hi) / 2;
      if (rp->bursts[mid].zone_first <= a) { ans = mid; lo = mid + 1; } else hi = mid - 1; }
   if (ans < 0) return -1;
   const rtfe_burst *B = &rp->bursts[ans];
   if ((B->flags & (RTFE_F_UNSAFE | RTFE_F_EVENT_OVERFLOW | RTFE_F_SCREEN_UNDERFLOW | RTFE_F_DETECTOR_FATAL)) || a > B->safe_last) return -1;
   return ans; }

static int burst_usable(const struct rt_replay *rp, int64_t b) {
   if (b < 0 || b >= rp->nbursts) return 0;
   return !(rp->bursts[b].flags & (RTFE_F_UNSAFE | RTFE_F_EVENT_OVERFLOW | RTFE_F_SCREEN_UNDERFLOW | RTFE_F_DETECTOR_FATAL)); }

void rt_replay_save_pos(void *ctx) {
   struct rt_replay *rp = (struct rt_replay *)ctx;
   rp->saved_pos = rp->pos; rp->saved_time = rp->d->timenow; }

void rt_replay_restore_pos(void *ctx) {
   struct rt_replay *rp = (struct rt_replay *)ctx;
   rp->pos = rp->saved_pos; rp->d->timenow = rp->saved_time; }

/* one transition, exactly as lookfor_peak/refine_peak hand it to process_*_transition */
static void deliver(struct rt_replay *rp, const struct evsrc *s, int trk, const rtfe_event *e, int W) {
   struct rt_dec *d = rp->d;
   struct rt_trk *t = &d->trk[trk];
   if (s->stride == sizeof(rtfe_ww_event) && rp->find_zeros) {
      /* Whirlwind (rtfe_ww_detector_scan): the same two deliveries from the wide record - offsets of any length and of either sign (nothing
       * restarts between blocks, and the -deskew rewind leaves pending rows AHEAD of the rows that confirm them), and for the differentiated
       * detector the opposite excursion as the reference holds it at the callback (src/decoder.c:663-667, 676-680: it zeroes it afterwards),
       * which the -deskew pre-pass reads (rt_decode_ww.c: v_top - v_bot per pulse end) */
      const rtfe_ww_event *we = (const rtfe_ww_event *)e;
      const int64_t row = s->reset + (int64_t)e->sample;
      if (d->opt.do_differentiate) {
         const double tz = we->has_zero ? (time_of_row(rp, row - we->back_first) + time_of_row(rp, row - we->back_last)) / 2
                                        : d->timenow - d->sample_deltat / 2;
         if (e->flags & 1) { t->v_bot = e->v_peak; t->v_top = we->v_other; t->t_bot = tz; rt_down_transition(d, t); }
         else { t->v_top = e->v_peak; t->v_bot = we->v_other; t->t_top = tz; rt_up_transition(d, t); }
         ++rp->events_delivered;
         return; }
      const double t_cross = time_of_row(rp, row - we->back_first);
      if (e->flags & 1) {
         t->v_bot = e->v_peak; t->t_bot = t_cross; t->v_top = 0;
         if (d->timenow - t->t_bot <= t->clkavg.t_bitspaceavg * 1.5f) { rt_down_transition(d, t); ++rp->events_delivered; } }
      else {
         t->v_top = e->v_peak; t->t_top = t_cross; t->v_bot = 0;
         if (d->timenow - t->t_top <= t->clkavg.t_bitspaceavg * 1.5f) { rt_up_transition(d, t); ++rp->events_delivered; } }
      return; }
   if (rp->find_zeros && d->opt.do_differentiate) {
      /* differentiated signal (src/decoder.c:657-663, 670-676): the crossing is the centre of the run of exact
       * zeros if there was one, else half a sample before the confirming row; no slope gate */
      uint32_t dd; memcpy(&dd, &e->agc_gain, 4);
      const int64_t row = s->reset + (int64_t)e->sample;
      const uint32_t d1 = dd >> 16, d2 = dd & 0xffff;
      const double tz = d1 ? ((double)(rp->tstart_ns + (row - d1) * rp->tdelta_ns) / 1e9 + (double)(rp->tstart_ns + (row - d2) * rp->tdelta_ns) / 1e9) / 2
                           : d->timenow - d->sample_deltat / 2;
      if (e->flags & 1) { t->v_bot = e->v_peak; t->t_bot = tz; rt_down_transition(d, t); }
      else { t->v_top = e->v_peak; t->t_top = tz; rt_up_transition(d, t); }
      ++rp->events_delivered;
      return; }
   if (rp->find_zeros) {
      /* a confirmed zero crossing (src/decoder.c:625-630, 639-644): the extreme is new, the opposite excursion
       * restarts, and the transition counts only if the excursion was reached soon enough after the crossing */
      uint32_t delay; memcpy(&delay, &e->agc_gain, 4);
      const int64_t cross_row = s->reset + (int64_t)e->sample - (int64_t)delay;
      const double t_cross = (double)(rp->tstart_ns + cross_row * rp->tdelta_ns) / 1e9;
      if (e->flags & 1) {
         t->v_bot = e->v_peak; t->t_bot = t_cross; t->v_top = 0;
         if (d->timenow - t->t_bot <= t->clkavg.t_bitspaceavg * 1.5f) { rt_down_transition(d, t); ++rp->events_delivered; } }
      else {
         t->v_top = e->v_peak; t->t_top = t_cross; t->v_bot = 0;
         if (d->timenow - t->t_top <= t->clkavg.t_bitspaceavg * 1.5f) { rt_up_transition(d, t); ++rp->events_delivered; } }
      return; }
   const int adjc = (e->flags >> 1) & 3;
   const float adj = adjc == 1 ? -0.5f : (adjc == 2 ? 0.5f : 0.0f);
   const double tp = d->timenow - ((float)(W - e->left_distance) - adj) * d->sample_deltat;   /* src/decoder.c:732 */
   uint32_t ga, gb;
   memcpy(&ga, &t->agc_gain, 4); memcpy(&gb, &e->agc_gain, 4);
   if (ga != gb) ++rp->agc_mismatches;        /* the device's AGC mirror and the decoder's own AGC must agree bit for bit */
   if (e->flags & 1) { t->v_bot = e->v_peak; t->t_bot = tp; rt_down_transition(d, t); }
   else { t->v_top = e->v_peak; t->t_top = tp; rt_up_transition(d, t); }
   ++rp->events_delivered; }

/* optional dump of what the decoders are handed, in the record format of oracle/ref_event_shim.c */
struct dump_rec { uint32_t kind, trk; int32_t peakcount, parmset; double t_peak; int64_t timenow_ns; float v_peak, agc_gain, v_avg_height; uint32_t pad; };
static void dump_transition(struct rt_dec *d, struct rt_trk *t, int is_top, void *user) {
   struct rt_replay *rp = (struct rt_replay *)user;
   struct dump_rec r; memset(&r, 0, sizeof r);
   r.kind = is_top ? 0 : 1; r.trk = (uint32_t)t->trknum; r.peakcount = t->peakcount; r.parmset = d->parmset;
   r.t_peak = is_top ? t->t_top : t->t_bot;
   r.timenow_ns = rp->tstart_ns + (rp->cur_row + 1) * rp->tdelta_ns;          /* the reference has already advanced it, src/readtape.c:1424 */
   r.v_peak = is_top ? t->v_top : t->v_bot; r.agc_gain = t->agc_gain; r.v_avg_height = t->v_avg_height;
   fwrite(&r, sizeof r, 1, rp->evtf); }
static void dump_attempt(struct rt_dec *d, void *user) {
   struct rt_replay *rp = (struct rt_replay *)user;
   struct dump_rec r; memset(&r, 0, sizeof r);
   r.kind = 2; r.parmset = d->parmset; r.timenow_ns = rp->tstart_ns + rp->pos * rp->tdelta_ns;
   fwrite(&r, sizeof r, 1, rp->evtf); }

static int readblock_once(void *ctx, int retry) {
   struct rt_replay *rp = (struct rt_replay *)ctx;
   struct rt_dec *d = rp->d;
   const int ntrks = rp->ntrks, parmset = d->parmset;
   const int W = rp->W[parmset];
   const int64_t s0 = rp->pos;
   const int64_t nrows = rp->nrows;
   int endfile = 0;
   (void)retry;
   ++rp->attempts;
   if (s0 >= nrows) { rt_finish_attempt(d); return 0; }     /* no row was processed: no forced end of block */
   if (s0 >= rp->stop_row) { rt_finish_attempt(d); return 0; }   /* fragment decode: the next attempt starts in a zone the next fragment owns */

   struct evsrc src;
   const long dump_pos = rp->evtf ? ftell(rp->evtf) : 0;      /* a restarted attempt rewinds the optional dump */
   /* ... and what a pre-pass accumulates ACROSS attempts (the -deskew peak statistics, the density histogram): the reference reads
    * the block once, a restarted attempt must not count its transitions twice (found by tests/stress_gpu.py, seed 810 tape 100:
    * the pre-pass had its 1000 transitions per track one block early) */
   const int prepass_stats = d->doing_deskew || d->doing_density_detection || d->want_peakstats;      /* (... and what --peakstats gathers across the whole decode) */
   __typeof__(d->peakstat) saved_peakstat; __typeof__(d->estden) saved_estden;
   if (prepass_stats) { saved_peakstat = d->peakstat; saved_estden = d->estden; }
   int64_t b = find_burst(rp, s0);
   rtfe_event *exact_events = NULL;
   int using_exact = 0;
   int restarted = 0;
   /* an exact scan covers this attempt only: up to the end of the device burst after the one s0 lies in,
    * extended (x4) in the rare case the attempt runs longer */
   int64_t exact_len = 1 << 16;
   {  /* first burst whose zone starts behind s0 (the table is ordered: binary search) */
      int64_t lo = 0, hi = rp->nbursts;
      while (lo < hi) { const int64_t mid = (lo + hi) / 2; if (rp->bursts[mid].zone_first - rp->row_base > s0) hi = mid; else lo = mid + 1; }
      if (lo < rp->nbursts) exact_len = rp->bursts[lo].end_sample - rp->row_base - s0; }
   if (exact_len < (1 << 12)) exact_len = 1 << 12;
restart:
   if (rp->evtf && (restarted || using_exact)) fseek(rp->evtf, dump_pos, SEEK_SET);
   if (prepass_stats && (restarted || using_exact)) { d->peakstat = saved_peakstat; d->estden = saved_estden; }
   if (b < 0) {                                               /* outside every proven-safe zone: exact device scan */
      if (!rp->exact) { ++rp->device_failures; d->results[parmset].blktype = RT_BS_ABORTED; rt_finish_attempt(d); return 0; }
      uint32_t cnt[RT_MAXTRKS]; rtfe_burst eb; uint32_t cap = 0;
      if (exact_events && rp->exact_free) { rp->exact_free(rp->exact_user, exact_events); exact_events = NULL; }
      const int64_t ex_end = s0 + exact_len < nrows ? s0 + exact_len : nrows;
      if (rp->exact(rp->exact_user, s0, ex_end, rp->find_zeros ? 0 : parmset, &eb, cnt, &exact_events, &cap) != 0) {
         ++rp->device_failures; d->results[parmset].blktype = RT_BS_ABORTED; rt_finish_attempt(d); return 0; }
      src.stride = sizeof(rtfe_event);
      for (int t = 0; t < ntrks; ++t) { src.list[t] = (const unsigned char *)(exact_events + (uint64_t)t * cap); src.n[t] = cnt[t]; src.at[t] = 0; }
      src.reset = s0; src.end = ex_end;
      for (int t = 0; t < ntrks; ++t) evsrc_sync(&src, t);
      using_exact = 1; ++rp->exact_scans; }
   else { evsrc_from_burst(&src, rp, b, parmset); evsrc_skip_before(&src, ntrks, s0); }

   int64_t events_seen = 0;
   int64_t row = s0;                 /* next row to "process" */
   int ntrk_started = 0;             /* tracks whose staggered start row has passed */
   for (;;) {
      /* ---- the next row at which anything can happen ---- */
      int64_t next = nrows;
      if (d->interblock_counter) {                          /* rows are skipped; the attempt returns when it reaches 0 */
         next = row + d->interblock_counter - 1; if (next > nrows) next = nrows; }
      else {
         if (ntrk_started < ntrks) { int64_t r = s0 + ntrk_started; if (r < next) next = r; }
         int64_t r = evsrc_next_row(&src, ntrks); if (r < next) next = r;
         if (d->opt.mode == RT_NRZI && d->nrzi.datablock && next > row && pred_nrzi(d, NULL, time_of_row(rp, next - 1))) {
            /* (the mid-bit timer is monotone in time: it can only run out before `next` if it has at row next - 1) */
            r = first_row_where(rp, pred_nrzi, NULL, d->nrzi.t_lastclock + 2 * d->nrzi.clkavg.t_bitspaceavg, row, next);
            if (r < next) next = r; }
         if (d->opt.mode == RT_PE)
            for (int t = 0; t < ntrks; ++t) {
               struct rt_trk *tk = &d->trk[t];
               if (!tk->idle && tk->t_lastpeak != 0) {
                  r = first_row_where(rp, pred_pe, tk, tk->t_lastpeak + tk->clkavg.t_bitspaceavg * 2.5f, row, next);
                  if (r < next) next = r; } }
         if (d->opt.mode == RT_GCR)
            for (int t = 0; t < ntrks; ++t) {
               struct rt_trk *tk = &d->trk[t];
               if (tk->datablock) {
                  r = first_row_where(rp, pred_gcr, tk, tk->t_lastpeak + 6.00 * tk->clkavg.t_bitspaceavg, row, next);
                  if (r < next) next = r; } } }
      /* the event source ends before anything else happens? */
      if (using_exact && !d->interblock_counter && next >= src.end && src.end < nrows) {
         exact_len *= 4;                                       /* the attempt is longer than the exact scan: rescan further */
         { void (*oa)(struct rt_dec *, void *) = d->on_attempt; d->on_attempt = NULL; rt_init_trackstate(d); d->on_attempt = oa; }
         d->interblock_counter = 0;
         goto restart; }
      if (!using_exact && !d->interblock_counter && next >= src.end && src.end < nrows) {
         /* still fresh: the next burst's fresh state is the same state.  During density detection the detector never
          * leaves its fresh AGC / baseline state (no decoder runs), so every proven restart is the same state */
         const int fresh = (events_seen == 0 || d->doing_density_detection)
                           && !(rp->find_zeros && (rp->bursts[b].flags & RTFE_F_STATE_AT_END));     /* (-zeros: an excursion without an event is history too) */
         if (fresh && rp->stop_row != INT64_MAX
             && (b + 1 >= rp->nbursts || rp->bursts[b + 1].zone_first - rp->row_base >= rp->stop_row)) {
            /* fragment decode: the burst behind this one belongs to the next fragment (it is the bounding entry of the table, or not in
             * it at all), whose replay starts from the same fresh state at the start of that burst's zone - this attempt saw nothing
             * and ends here without a block.  (chaining on, or redoing the attempt from an exact scan, decoded the
             * neighbour's block a second time.) */
            rp->pos = rp->stop_row;
            rt_finish_attempt(d);
            return 0; }
         if (fresh && burst_usable(rp, b + 1)) {
            ++b; evsrc_from_burst(&src, rp, b, parmset); evsrc_skip_before(&src, ntrks, row); ++rp->chained;
            continue; }
         if (restarted) { ++rp->device_failures; d->results[parmset].blktype = RT_BS_ABORTED; break; }
         /* this attempt crosses a device restart with state: redo it from s0 with an exact scan */
         restarted = 1; b = -1;
         { void (*oa)(struct rt_dec *, void *) = d->on_attempt; d->on_attempt = NULL; rt_init_trackstate(d); d->on_attempt = oa; }
         d->interblock_counter = 0;
         goto restart; }
      if (next >= nrows) {                                   /* end of data, src/readtape.c:1410-1413 */
         d->timenow = time_of_row(rp, nrows - 1);
         rt_force_end_of_block(d);
         rp->pos = nrows;
         endfile = 1;
         break; }
      row = next;
      rp->cur_row = row;
      d->timenow = time_of_row(rp, row);
      /* ---- process_sample for this row (src/decoder.c:841-904) ---- */
      if (d->interblock_counter) {                          /* we jumped to the row on which the countdown ends */
         d->interblock_counter = 0;
         rp->pos = row + 1;
         break; }
      if (d->opt.mode == RT_NRZI && rt_nrzi_zerocheck_due(d)) rt_nrzi_zerocheck(d);
      int stop_row = 0;
      for (int t = 0; t < ntrks && !stop_row; ++t) {
         struct rt_trk *tk = &d->trk[t];
         if (tk->t_lastpeak == 0) {                          /* first row of this track, src/decoder.c:855-861 */
            tk->v_lastpeak = 0;
            tk->t_lastpeak = d->timenow;
            if (t >= ntrk_started) ntrk_started = t + 1;
            break; }
         while (src.nr[t] == row) {
            if (evsrc_ev(&src, t, src.at[t])->flags & RTFE_EV_FATAL) {    /* "AGC gain bad in lookfor_peak" (src/decoder.c:782): the reference exits here */
               rp->reference_fatal = 1; d->fatal = 1; rp->fatal_row = row; rp->fatal_trk = t;
               d->results[parmset].blktype = RT_BS_ABORTED;
               if (exact_events && rp->exact_free) rp->exact_free(rp->exact_user, exact_events);
               rt_finish_attempt(d);
               return 0; }
            deliver(rp, &src, t, evsrc_ev(&src, t, src.at[t]), W);
            if (d->fatal) {                                      /* the decoder's callback met one of the reference's asserts (a learned peak height that is not positive): the run ends inside it */
               rp->reference_fatal = 1; rp->fatal_row = row; rp->fatal_trk = t;
               d->results[parmset].blktype = RT_BS_ABORTED;
               if (exact_events && rp->exact_free) rp->exact_free(rp->exact_user, exact_events);
               rt_finish_attempt(d);
               return 0; }
            ++src.at[t]; ++events_seen; evsrc_sync(&src, t); }
         if (d->opt.mode == RT_PE && rt_pe_idle_due(d, tk)) rt_pe_go_idle(d, tk);
         if (d->opt.mode == RT_GCR && rt_gcr_idle_due(d, tk)) if (rt_gcr_go_idle(d, tk)) stop_row = 1; }
      /* events of tracks the reference did not reach on this row cannot exist; drop anything stale */
      evsrc_skip_before(&src, ntrks, row + 1);
      /* exit: (src/decoder.c:900-904) */
      if (d->interblock_counter) {
         if (--d->interblock_counter) { ++row; continue; }
         rp->pos = row + 1; break; }
      if (d->results[parmset].blktype != RT_BS_NONE) { rp->pos = row + 1; break; }
      ++row; }
   if (exact_events && rp->exact_free) rp->exact_free(rp->exact_user, exact_events);
   rt_finish_attempt(d);
   return !endfile; }

int rt_replay_readblock(void *ctx, int retry) {
   struct rt_replay *rp = (struct rt_replay *)ctx;
   const int64_t from = rp->pos;
   const int more = readblock_once(ctx, retry);
   /* src/readtape.c:1404 counts every pass of the read loop of a first attempt, the one that finds the end marker included */
   if (!retry) rp->d->lines_in += (rp->pos - from) + (more ? 0 : 1);
   if (!retry && !more) rp->end_counted = 1;
   return more; }

/* ---- the text file of the next decode (-textfile): asked for by rt_replay_set_text on the calling thread, taken by the run that
 * processes blocks (not by a pre-pass), closed with its trailer when that run ends ---- */
static __thread struct { int set; rt_text_options o; char base[1024], created[64]; } g_text_request;
void rt_replay_set_text(const rt_text_options *o, const char *base, const char *created) {
   g_text_request.set = 0;
   if (!o || !base) return;
   g_text_request.o = *o;
   snprintf(g_text_request.base, sizeof g_text_request.base, "%s", base);
   snprintf(g_text_request.created, sizeof g_text_request.created, "%s", created ? created : "");
   g_text_request.set = 1; }
static void text_record_hook(void *t, const unsigned char *bytes, int length, int errs, int warnings, const char *head) {
   rt_text_record((struct rt_textfile *)t, bytes, length, errs, warnings, head); }
static void text_tapemark_hook(void *t, double timenow) { rt_text_tapemark((struct rt_textfile *)t, timenow); }
static struct rt_textfile *text_attach(struct rt_dec *d) {
   if (!g_text_request.set) return NULL;
   g_text_request.set = 0;
   g_text_request.o.ntrks = d->opt.ntrks;
   struct rt_textfile *t = rt_text_new(g_text_request.base, &g_text_request.o, 0, g_text_request.created[0] ? g_text_request.created : NULL);
   if (!t) return NULL;
   d->text = t; d->text_name = rt_text_filename(t); d->text_record = text_record_hook; d->text_tapemark = text_tapemark_hook;
   return t; }

/* ---- the flux-transition statistics of the next decode (<base>.peakstats.csv, <base>.peakstats_deskew.csv and the head-skew verdict): asked for by
 * rt_replay_set_peakstats on the calling thread.  A -deskew pre-pass on this thread reads the request and leaves what it learned (the largest delay as
 * a percentage of a bit, its histogram) with it; the run that processes blocks takes it.  Fragments never do: the bins are fixed by the tape's first
 * recorded transition, which only the first fragment sees. ---- */
struct peak_result { int valid, ok; float peak_frac, stddev_frac, leftbin, binwidth; int counts[RT_MAXTRKS][RT_PEAKSTAT_BUCKETS], trksums[RT_MAXTRKS]; };
static __thread struct { int set, quiet, deskew; char base[1024]; float deskew_pct; struct peak_result res[2]; } g_peak_request;
void rt_replay_set_peakstats(const char *base, int quiet, int deskew) {
   memset(&g_peak_request, 0, sizeof g_peak_request);
   if (!base) return;
   snprintf(g_peak_request.base, sizeof g_peak_request.base, "%s", base);
   g_peak_request.quiet = quiet; g_peak_request.deskew = deskew;
   g_peak_request.set = 1; }
int rt_replay_get_peakstats(int which, float *leftbin, float *binwidth, int32_t *counts, int32_t *trksums, int *ok, float *peak_frac, float *stddev_frac) {
   if (which < 0 || which > 1 || !g_peak_request.res[which].valid) return 0;
   const struct peak_result *r = &g_peak_request.res[which];
   *leftbin = r->leftbin; *binwidth = r->binwidth; *ok = r->ok; *peak_frac = r->peak_frac; *stddev_frac = r->stddev_frac;
   memcpy(counts, r->counts, sizeof r->counts); memcpy(trksums, r->trksums, sizeof r->trksums);
   return 1; }
static int peak_attach(struct rt_dec *d) {                       /* both passes: the decoders record, the files are named */
   if (!g_peak_request.set) return 0;
   d->want_peakstats = 1; d->peak_quiet = g_peak_request.quiet; d->peak_deskew = g_peak_request.deskew;
   snprintf(d->peak_base, sizeof d->peak_base, "%s", g_peak_request.base);
   d->deskew_max_delay_percent = g_peak_request.deskew_pct;
   return 1; }
static void peak_keep(struct rt_dec *d, int which) {
   struct peak_result *r = &g_peak_request.res[which];
   r->valid = 1; r->ok = d->skew_verdict.ok; r->peak_frac = d->skew_verdict.peak_frac; r->stddev_frac = d->skew_verdict.stddev_frac;
   r->leftbin = d->peakstat.leftbin; r->binwidth = d->peakstat.binwidth;
   memcpy(r->counts, d->peakstat.counts, sizeof r->counts); memcpy(r->trksums, d->peakstat.trksums, sizeof r->trksums);
   g_peak_request.deskew_pct = d->deskew_max_delay_percent; }
static void peak_report(struct rt_dec *d) {                      /* under the summary (src/readtape.c:2045-2058); the request is used up */
   rt_peakstats_report(d);
   peak_keep(d, 0);
   g_peak_request.set = 0; }

/* ---------------------------------------------------------------------------------------------------------------------
 * The block journal: a fragment's replay in journal mode puts no block out.  Where rt_process_blocks would call rt_got_tapemark /
 * rt_got_datablock it appends a record of what those read from the context; the finisher (below, behind the fragment runners) takes the fragments'
 * journals in tape order, puts each record back into ONE context and calls them there - block and file numbers, label state, the text file, -blklimit,
 * the counters of the summary are sequential across the tape, and there is one copy of the output stage.  The format is private: host-endian structs in
 * memory, read by nobody else.  (The PE, NRZI and GCR decoders write no log lines of their own; Whirlwind's, which do, is not decoded in fragments.)
 * --------------------------------------------------------------------------------------------------------------------- */
struct rt_peakbins { pthread_mutex_t mu; int have; float leftbin, binwidth; };      /* the histogram's bins, shared by a tape's fragments and its finisher */
struct peak_raw { float bitspacing, peaktime; int32_t trk; };                        /* a transition recorded while the bins were not known */
struct peak_counts { int32_t initialized; int32_t counts[RT_MAXTRKS][RT_PEAKSTAT_BUCKETS], trksums[RT_MAXTRKS]; int64_t nraw; };
struct journal_work { int64_t attempts, exact_scans, chained, events_delivered, agc_mismatches; };
#define JREC_MAGIC 0x4a524543u
struct jrec {                      /* followed by ndata + nfaked uint16 words (the data, parity bit included; PE: the faked bits), then with has_snap a peak_counts */
   uint32_t magic; int32_t blktype, parmset, tries, ndata, nfaked, all_clean, goodmultiple, has_snap, pad;
   double timenow, t_blockstart;
   int64_t end_abs, lines_in;                                 /* the absolute row behind the block's last attempt; the fragment's lines_in so far */
   struct journal_work work;                                  /* the replay's counters so far */
   int32_t tried[RT_MAXPARMSETS], chosen[RT_MAXPARMSETS];      /* so far, in this fragment */
   struct rt_results res; };
struct rt_journal {
   unsigned char *buf; size_t len, cap; int nrec, failed;
   struct rt_peakbins *bins; int first, snapshots;            /* bins != NULL: the fragment gathers peak statistics; first: it is the tape's first fragment */
   struct peak_raw *raw; int64_t raw_cap;
   /* what the fragment's replay left when it ended */
   int done, all_clean, end_counted;
   int64_t start_abs, final_abs, lines_in; double timenow;
   int32_t tried[RT_MAXPARMSETS], chosen[RT_MAXPARMSETS], goodmultiple;
   struct rt_replay_stats stats; struct peak_counts peak; };
struct journal_hook { struct rt_journal *j; struct rt_replay *rp; };

struct rt_peakbins *rt_peakbins_new(void) {
   struct rt_peakbins *b = (struct rt_peakbins *)calloc(1, sizeof *b);
   if (b) pthread_mutex_init(&b->mu, NULL);
   return b; }
void rt_peakbins_free(struct rt_peakbins *b) { if (b) { pthread_mutex_destroy(&b->mu); free(b); } }

struct rt_journal *rt_journal_new(struct rt_peakbins *bins, int first, int snapshots) {
   struct rt_journal *j = (struct rt_journal *)calloc(1, sizeof *j);
   if (j) { j->bins = bins; j->first = first; j->snapshots = snapshots && bins; j->all_clean = 1; }
   return j; }
void rt_journal_free(struct rt_journal *j) { if (j) { free(j->buf); free(j->raw); free(j); } }
int64_t rt_journal_bytes(const struct rt_journal *j) { return j ? (int64_t)(j->len + (size_t)j->raw_cap * sizeof(struct peak_raw)) : 0; }
int rt_journal_records(const struct rt_journal *j) { return j ? j->nrec : 0; }
int64_t rt_journal_final_row(const struct rt_journal *j) { return j && j->done ? j->final_abs : -1; }
int rt_journal_stats(const struct rt_journal *j, struct rt_replay_stats *stats) { if (!j || !j->done || !stats) return -1; *stats = j->stats; return 0; }

static void journal_put(struct rt_journal *j, const void *p, size_t n) {
   if (j->failed) return;
   if (j->len + n > j->cap) {
      size_t cap = j->cap ? j->cap : 4096;
      while (cap < j->len + n) cap *= 2;
      unsigned char *nb = (unsigned char *)realloc(j->buf, cap);
      if (!nb) { j->failed = 1; return; }
      j->buf = nb; j->cap = cap; }
   if (n) memcpy(j->buf + j->len, p, n);
   j->len += n; }

static void peak_counts_of(const struct rt_dec *d, struct peak_counts *p) {
   p->initialized = d->peakstat.initialized; p->nraw = d->peakstat.nraw;
   memcpy(p->counts, d->peakstat.counts, sizeof p->counts); memcpy(p->trksums, d->peakstat.trksums, sizeof p->trksums); }

/* One block of the context `d` into the journal.  end_abs / work: what the replay knows (rt_journal_record: a caller without a replay gives zeros) */
static void journal_record(struct rt_journal *j, struct rt_dec *d, enum rt_bstate blktype, int64_t end_abs, const struct journal_work *work) {
   const struct rt_results *res = &d->results[d->parmset];
   struct jrec r; memset(&r, 0, sizeof r);
   r.magic = JREC_MAGIC; r.blktype = (int32_t)blktype; r.parmset = d->parmset; r.tries = d->tries;
   r.ndata = blktype == RT_BS_BLOCK && res->minbits > 0 ? (res->minbits < RT_MAXBLOCK ? res->minbits : RT_MAXBLOCK) : 0;
   r.nfaked = d->opt.mode == RT_PE ? r.ndata : 0;             /* (format_block_errors counts them) */
   r.all_clean = d->run_all_clean; r.goodmultiple = d->numblks_goodmultiple; r.has_snap = j->snapshots;
   r.timenow = d->timenow; r.t_blockstart = d->t_blockstart; r.end_abs = end_abs; r.lines_in = d->lines_in;
   if (work) r.work = *work;
   for (int i = 0; i < RT_MAXPARMSETS; ++i) { r.tried[i] = d->parmsets[i].tried; r.chosen[i] = d->parmsets[i].chosen; }
   r.res = *res;
   journal_put(j, &r, sizeof r);
   journal_put(j, d->data, sizeof(uint16_t) * (size_t)r.ndata);
   journal_put(j, d->data_faked, sizeof(uint16_t) * (size_t)r.nfaked);
   if (r.has_snap) { struct peak_counts p; memset(&p, 0, sizeof p); peak_counts_of(d, &p); journal_put(j, &p, sizeof p); }
   ++j->nrec; }
void rt_journal_record(struct rt_journal *j, struct rt_dec *d, int blktype) { journal_record(j, d, (enum rt_bstate)blktype, 0, NULL); }
void rt_journal_close(struct rt_journal *j) { if (j) { j->done = 1; j->all_clean = 1; } }

static void journal_on_block(struct rt_dec *d, enum rt_bstate blktype, void *user) {
   struct journal_hook *h = (struct journal_hook *)user;
   const struct rt_replay *rp = h->rp;
   const struct journal_work w = { rp->attempts, rp->exact_scans, rp->chained, rp->events_delivered, rp->agc_mismatches };
   journal_record(h->j, d, blktype, rp->pos + rp->row_base, &w); }

/* a transition while the fragment does not know the bins: the tape's first fragment fixes and publishes them, any other takes what is published - or
 * keeps the transition until somebody has published (it never waits: the fragments may run in any order, on any number of threads, and the finisher,
 * which goes through the journals in tape order, fixes the bins itself where a journal still holds transitions and nobody has) */
static int journal_unbinned(struct rt_dec *d, float bitspacing, float peaktime, int trknum) {
   struct rt_journal *j = (struct rt_journal *)d->peak_user;
   struct rt_peakbins *B = j->bins;
   float left, bw;
   pthread_mutex_lock(&B->mu);
   if (!B->have && j->first) { rt_peakstat_bins(d->opt.mode, bitspacing, &B->leftbin, &B->binwidth); B->have = 1; }
   const int have = B->have;
   left = B->leftbin; bw = B->binwidth;
   pthread_mutex_unlock(&B->mu);
   if (!have) {
      if (d->peakstat.nraw >= j->raw_cap) {
         const int64_t cap = j->raw_cap ? j->raw_cap * 2 : 4096;
         struct peak_raw *nr = (struct peak_raw *)realloc(j->raw, sizeof(struct peak_raw) * (size_t)cap);
         if (!nr) { j->failed = 1; return 0; }
         j->raw = nr; j->raw_cap = cap; }
      const struct peak_raw r = { bitspacing, peaktime, trknum };
      j->raw[d->peakstat.nraw++] = r;
      return 0; }
   const int64_t n = d->peakstat.nraw;                        /* (an attempt's roll-back may bring them back: they stay where they are) */
   rt_peakstat_start(d, left, bw);
   for (int64_t i = 0; i < n; ++i) rt_peakstat_count(d, j->raw[i].peaktime, j->raw[i].trk);
   return 1; }

static void journal_attach(struct rt_dec *d, struct journal_hook *h) {
   d->on_block = journal_on_block; d->on_block_user = h;
   h->j->start_abs = h->rp->pos + h->rp->row_base;
   if (h->j->bins) { d->want_peakstats = 1; d->peak_unbinned = journal_unbinned; d->peak_user = h->j; } }

static void journal_close(struct rt_dec *d, struct journal_hook *h, int ok) {
   struct rt_journal *j = h->j;
   const struct rt_replay *rp = h->rp;
   j->done = 1; j->all_clean = ok; j->end_counted = rp->end_counted;
   j->final_abs = rp->pos + rp->row_base; j->lines_in = d->lines_in; j->timenow = d->timenow; j->goodmultiple = d->numblks_goodmultiple;
   for (int i = 0; i < RT_MAXPARMSETS; ++i) { j->tried[i] = d->parmsets[i].tried; j->chosen[i] = d->parmsets[i].chosen; }
   peak_counts_of(d, &j->peak); }

/* prepass != NULL: run the -deskew pre-pass instead of the decode (no .tap); append: keep what is already in the log
 * and event-dump files (the decode that follows a pre-pass continues both, as the reference's single run does) */
struct deskew_out { int *delays; int *nblks; int *hit_end; float *bpi, *implied; };
static int replay_any(const struct rt_options *opt, const struct rt_parms *parmsets, int nparm,
                  int64_t tdelta_ns, int64_t tstart_ns, int64_t nrows, int64_t row_base, const int *W,
                  const rtfe_burst *bursts, int64_t nbursts, const uint32_t *counts, const rtfe_event *events,
                  rt_exact_fn exact, rt_exact_free_fn exact_free, void *user,
                  const char *tap_path, const char *log_path, const char *evt_path, struct rt_replay_stats *stats,
                  int append, struct deskew_out *prepass, int64_t start_row, int64_t stop_row, int fragment,
                  const char *out_base, const char *in_name, struct rt_journal *jr) {
   const float sample_deltat = (float)tdelta_ns / 1e9f;              /* src/readtape.c:1345 */
   struct rt_dec *d = rt_dec_new(opt, sample_deltat, tdelta_ns);
   if (!d) return -1;
   if (parmsets) {
      memset(d->parmsets, 0, sizeof d->parmsets);
      memcpy(d->parmsets, parmsets, sizeof(struct rt_parms) * (size_t)nparm); }
   else for (int i = nparm; i < RT_MAXPARMSETS; ++i) d->parmsets[i].active = 0;   /* only the scanned sets are usable */
   if (out_base) snprintf(d->outbase, sizeof d->outbase, "%s", out_base);      /* files by the reference's names, made when first needed */
   else if (tap_path) d->tapf = fopen(tap_path, "wb");
   if (log_path) d->logf = fopen(log_path, append ? "a" : "w");
   const double wall0 = (double)time(NULL);
   struct rt_replay rp; memset(&rp, 0, sizeof rp);
   rp.d = d; rp.ntrks = opt->ntrks; rp.nparm = nparm;
   for (int i = 0; i < nparm; ++i) rp.W[i] = W[i];
   rp.nrows = nrows; rp.row_base = row_base; rp.tstart_ns = tstart_ns; rp.tdelta_ns = tdelta_ns;
   if (jr) rp.tstart_ns += row_base * tdelta_ns;      /* journal mode: the tape's own times (they are logged); a fragment's piece of a .tap holds none, and its clock starts with it */
   rp.bursts = bursts; rp.nbursts = nbursts; rp.counts = counts; rp.events = events;
   rp.exact = exact; rp.exact_free = exact_free; rp.exact_user = user;
   rp.find_zeros = opt->find_zeros;
   rp.pos = start_row; rp.stop_row = stop_row;
   d->no_tap_end = fragment;                      /* a fragment's .tap is concatenated with its neighbours': the caller ends the file */
   if (evt_path) {
      /* (not "ab": a restarted attempt rewinds the dump, and O_APPEND ignores seeks) */
      rp.evtf = append ? fopen(evt_path, "r+b") : fopen(evt_path, "wb");
      if (rp.evtf && append) fseek(rp.evtf, 0, SEEK_END);
      if (rp.evtf) { d->on_transition = dump_transition; d->on_attempt = dump_attempt; d->user = &rp; } }
   struct rt_reader rd = { rt_replay_readblock, rt_replay_save_pos, rt_replay_restore_pos, &rp };
   int ok = 1;
   int peaks = 0;
   if (prepass && prepass->bpi) *prepass->bpi = rt_density_prepass(d, &rd, prepass->implied, prepass->nblks, prepass->hit_end);
   else if (prepass) {
      peaks = peak_attach(d);
      *prepass->nblks = rt_deskew_prepass(d, &rd, prepass->delays, prepass->hit_end);
      if (peaks && *prepass->nblks >= 0) peak_keep(d, 1); }
   else {
      if (!fragment) peaks = peak_attach(d);
      struct rt_textfile *text = jr ? NULL : text_attach(d);
      struct journal_hook jh = { jr, &rp };
      if (jr) journal_attach(d, &jh);
      ok = rt_process_blocks(d, &rd, 0x7fffffff);
      if (jr) journal_close(d, &jh, ok);
      if (text) { d->text = NULL; d->text_record = NULL; d->text_tapemark = NULL; rt_text_close(text, 1); } }      /* src/readtape.c:1886 */
   if (in_name && !prepass) rt_write_summary(d, in_name, difftime(time(NULL), (time_t)wall0));
   if (peaks && !prepass) peak_report(d);
   if (stats) {
      stats->attempts = rp.attempts; stats->exact_scans = rp.exact_scans; stats->chained = rp.chained;
      stats->events_delivered = rp.events_delivered; stats->agc_mismatches = rp.agc_mismatches;
      stats->blocks = d->numblks; stats->tapemarks = d->numtapemarks; stats->blocks_with_errors = d->numblks_err;
      stats->blocks_with_warnings = d->numblks_warn; stats->blocks_unusable = d->numblks_unusable; stats->all_ok = ok;
      stats->data_bytes = d->numdatabytes; stats->device_failures = rp.device_failures;
      stats->reference_fatal = rp.reference_fatal; stats->fatal_row = rp.fatal_row; stats->fatal_trk = rp.fatal_trk; }
   if (d->tapf) fclose(d->tapf);
   if (d->logf) fclose(d->logf);
   if (rp.evtf) { fflush(rp.evtf); if (ftruncate(fileno(rp.evtf), ftell(rp.evtf))) {} fclose(rp.evtf); }
   rt_dec_free(d);
   return (prepass && rp.reference_fatal) ? -3 : 0; }      /* (a pre-pass has no statistics to carry it: the reference died inside the pre-pass) */

int rt_replay_run(const struct rt_options *opt, const struct rt_parms *parmsets, int nparm,
                  int64_t tdelta_ns, int64_t tstart_ns, int64_t nrows, int64_t row_base, const int *W,
                  const rtfe_burst *bursts, int64_t nbursts, const uint32_t *counts, const rtfe_event *events,
                  rt_exact_fn exact, rt_exact_free_fn exact_free, void *user,
                  const char *tap_path, const char *log_path, const char *evt_path, struct rt_replay_stats *stats) {
   return replay_any(opt, parmsets, nparm, tdelta_ns, tstart_ns, nrows, row_base, W, bursts, nbursts, counts, events,
                     exact, exact_free, user, tap_path, log_path, evt_path, stats, 0, NULL, 0, INT64_MAX, 0, NULL, NULL, NULL); }

/* One fragment of a tape (a time shard, or one window of a streamed file): rows are relative to the fragment's first row
 * (row_base = its absolute index; the bursts carry absolute rows).  The decode starts at start_row (0, or the start of the zone
 * in front of the fragment's first own burst: any start inside a zone is the same detector state) and ends when an
 * attempt would start at or behind stop_row (the start of the first zone the next fragment owns; INT64_MAX: run to the end of
 * the data).  No end-of-medium marker is written: the fragments' .tap files are concatenated by the caller. */
int rt_replay_run_fragment(const struct rt_options *opt, const struct rt_parms *parmsets, int nparm,
                  int64_t tdelta_ns, int64_t tstart_ns, int64_t nrows, int64_t row_base, const int *W,
                  const rtfe_burst *bursts, int64_t nbursts, const uint32_t *counts, const rtfe_event *events,
                  rt_exact_fn exact, rt_exact_free_fn exact_free, void *user,
                  const char *tap_path, const char *log_path, const char *evt_path, struct rt_replay_stats *stats,
                  int64_t start_row, int64_t stop_row) {
   return replay_any(opt, parmsets, nparm, tdelta_ns, tstart_ns, nrows, row_base, W, bursts, nbursts, counts, events,
                     exact, exact_free, user, tap_path, log_path, evt_path, stats, 0, NULL, start_row, stop_row, 1, NULL, NULL, NULL); }

/* ---- fragments side by side: native threads (the caller is one Python thread per window, not one per fragment) ---- */
struct frag_job {
   const struct rt_options *opt; const struct rt_parms *parmsets; int nparm; int64_t tdelta_ns, tstart_ns, nrows, row_base; const int *W;
   const rtfe_burst *bursts; int64_t nbursts; const uint32_t *counts; const rtfe_event *events;
   rt_exact_fn exact; rt_exact_free_fn exact_free; void *user;
   const char *tap_path; int64_t start_row, stop_row; struct rt_replay_stats *stats; double *seconds; int rc; struct rt_journal *journal; };
static void *frag_thread(void *p) {
   struct frag_job *j = (struct frag_job *)p;
   struct timespec a, b;
   clock_gettime(CLOCK_MONOTONIC, &a);
   if (j->journal)                                              /* journal mode: no piece of the .tap, the blocks go into the fragment's journal */
      j->rc = replay_any(j->opt, j->parmsets, j->nparm, j->tdelta_ns, j->tstart_ns, j->nrows, j->row_base, j->W, j->bursts, j->nbursts, j->counts, j->events,
                         j->exact, j->exact_free, j->user, NULL, NULL, NULL, &j->journal->stats, 0, NULL, j->start_row, j->stop_row, 1, NULL, NULL, j->journal);
   else
      j->rc = rt_replay_run_fragment(j->opt, j->parmsets, j->nparm, j->tdelta_ns, j->tstart_ns, j->nrows, j->row_base, j->W, j->bursts, j->nbursts, j->counts, j->events,
                                     j->exact, j->exact_free, j->user, j->tap_path, NULL, NULL, j->stats, j->start_row, j->stop_row);
   clock_gettime(CLOCK_MONOTONIC, &b);
   *j->seconds = (double)(b.tv_sec - a.tv_sec) + 1e-9 * (double)(b.tv_nsec - a.tv_nsec);
   return NULL; }
static int run_fragments(const struct rt_options *opt, const struct rt_parms *parmsets, int nparm,
                  int64_t tdelta_ns, int64_t tstart_ns, int64_t nrows, int64_t row_base, const int *W,
                  const rtfe_burst *bursts, int64_t nbursts, const uint32_t *counts, const rtfe_event *events,
                  rt_exact_fn exact, rt_exact_free_fn exact_free, void *user,
                  int nfrag, const char *const *tap_paths, struct rt_journal *const *journals, const int64_t *start_rows, const int64_t *stop_rows,
                  struct rt_replay_stats *stats, double *seconds) {
   if (nfrag < 1 || nfrag > 256) return -1;
   struct frag_job *jobs = (struct frag_job *)calloc((size_t)nfrag, sizeof *jobs);
   pthread_t *th = (pthread_t *)calloc((size_t)nfrag, sizeof *th);
   if (!jobs || !th) { free(jobs); free(th); return -1; }
   for (int i = 0; i < nfrag; ++i) {
      struct frag_job j = { opt, parmsets, nparm, tdelta_ns, tstart_ns, nrows, row_base, W, bursts, nbursts, counts, events, exact, exact_free, user,
                            tap_paths ? tap_paths[i] : NULL, start_rows[i], stop_rows[i], stats ? &stats[i] : NULL, &seconds[i], 0, journals ? journals[i] : NULL };
      jobs[i] = j; }
   int started = 0, rc = 0;
   for (int i = 1; i < nfrag; ++i) { if (pthread_create(&th[i], NULL, frag_thread, &jobs[i]) != 0) break; started = i; }
   frag_thread(&jobs[0]);                                       /* (the caller's thread takes the first) */
   for (int i = started + 1; i < nfrag; ++i) frag_thread(&jobs[i]);      /* (threads that could not be made: in line) */
   for (int i = 1; i <= started; ++i) pthread_join(th[i], NULL);
   for (int i = 0; i < nfrag; ++i) if (jobs[i].rc != 0 && rc == 0) rc = jobs[i].rc;
   free(jobs); free(th);
   return rc; }
int rt_replay_run_fragments(const struct rt_options *opt, const struct rt_parms *parmsets, int nparm,
                  int64_t tdelta_ns, int64_t tstart_ns, int64_t nrows, int64_t row_base, const int *W,
                  const rtfe_burst *bursts, int64_t nbursts, const uint32_t *counts, const rtfe_event *events,
                  rt_exact_fn exact, rt_exact_free_fn exact_free, void *user,
                  int nfrag, const char *const *tap_paths, const int64_t *start_rows, const int64_t *stop_rows, struct rt_replay_stats *stats, double *seconds) {
   return run_fragments(opt, parmsets, nparm, tdelta_ns, tstart_ns, nrows, row_base, W, bursts, nbursts, counts, events, exact, exact_free, user,
                        nfrag, tap_paths, NULL, start_rows, stop_rows, stats, seconds); }
int rt_replay_journal_fragments(const struct rt_options *opt, const struct rt_parms *parmsets, int nparm,
                  int64_t tdelta_ns, int64_t tstart_ns, int64_t nrows, int64_t row_base, const int *W,
                  const rtfe_burst *bursts, int64_t nbursts, const uint32_t *counts, const rtfe_event *events,
                  rt_exact_fn exact, rt_exact_free_fn exact_free, void *user,
                  int nfrag, struct rt_journal *const *journals, const int64_t *start_rows, const int64_t *stop_rows, double *seconds) {
   for (int i = 0; i < nfrag; ++i) if (!journals[i]) return -1;
   return run_fragments(opt, parmsets, nparm, tdelta_ns, tstart_ns, nrows, row_base, W, bursts, nbursts, counts, events, exact, exact_free, user,
                        nfrag, NULL, journals, start_rows, stop_rows, NULL, seconds); }

struct read_job { int fd; char *dst; int64_t off, n; int rc; };
static void *read_thread(void *p) {
   struct read_job *j = (struct read_job *)p;
   int64_t done = 0;
   while (done < j->n) {
      const int64_t want = j->n - done > (1ll << 30) ? (1ll << 30) : j->n - done;
      const ssize_t got = pread(j->fd, j->dst + done, (size_t)want, (off_t)(j->off + done));
      if (got <= 0) { j->rc = -1; return NULL; }
      done += got; }
   return NULL; }
int rt_read_mt(int fd, void *dst, int64_t off, int64_t nbytes, int nthreads) {
   if (nbytes <= 0) return 0;
   if (nthreads < 1) nthreads = 1;
   if (nthreads > 64) nthreads = 64;
   if (nbytes < (8ll << 20)) nthreads = 1;
   struct read_job jobs[64];
   pthread_t th[64];
   const int64_t step = ((nbytes + nthreads - 1) / nthreads + 4095) & ~4095ll;
   int n = 0;
   for (int64_t a = 0; a < nbytes; a += step, ++n) { struct read_job j = { fd, (char *)dst + a, off + a, nbytes - a < step ? nbytes - a : step, 0 }; jobs[n] = j; }
   int started = 0;
   for (int i = 1; i < n; ++i) { if (pthread_create(&th[i], NULL, read_thread, &jobs[i]) != 0) break; started = i; }
   read_thread(&jobs[0]);
   for (int i = started + 1; i < n; ++i) read_thread(&jobs[i]);
   for (int i = 1; i <= started; ++i) pthread_join(th[i], NULL);
   for (int i = 0; i < n; ++i) if (jobs[i].rc != 0) return -1;
   return 0; }

int rt_replay_run_after_deskew(const struct rt_options *opt, const struct rt_parms *parmsets, int nparm,
                  int64_t tdelta_ns, int64_t tstart_ns, int64_t nrows, int64_t row_base, const int *W,
                  const rtfe_burst *bursts, int64_t nbursts, const uint32_t *counts, const rtfe_event *events,
                  rt_exact_fn exact, rt_exact_free_fn exact_free, void *user,
                  const char *tap_path, const char *log_path, const char *evt_path, struct rt_replay_stats *stats) {
   return replay_any(opt, parmsets, nparm, tdelta_ns, tstart_ns, nrows, row_base, W, bursts, nbursts, counts, events,
                     exact, exact_free, user, tap_path, log_path, evt_path, stats, 1, NULL, 0, INT64_MAX, 0, NULL, NULL, NULL); }

int rt_replay_deskew(const struct rt_options *opt, const struct rt_parms *parmsets, int nparm,
                  int64_t tdelta_ns, int64_t tstart_ns, int64_t nrows, int64_t row_base, const int *W,
                  const rtfe_burst *bursts, int64_t nbursts, const uint32_t *counts, const rtfe_event *events,
                  rt_exact_fn exact, rt_exact_free_fn exact_free, void *user,
                  const char *log_path, const char *evt_path, int append, int *delays, int *nblks, int *hit_end) {
   struct deskew_out o = { delays, nblks, hit_end, NULL, NULL };
   return replay_any(opt, parmsets, nparm, tdelta_ns, tstart_ns, nrows, row_base, W, bursts, nbursts, counts, events,
                     exact, exact_free, user, NULL, log_path, evt_path, NULL, append, &o, 0, INT64_MAX, 0, NULL, NULL, NULL); }


int rt_replay_density(const struct rt_options *opt, const struct rt_parms *parmsets, int nparm,
                  int64_t tdelta_ns, int64_t tstart_ns, int64_t nrows, int64_t row_base, const int *W,
                  const rtfe_burst *bursts, int64_t nbursts, const uint32_t *counts, const rtfe_event *events,
                  rt_exact_fn exact, rt_exact_free_fn exact_free, void *user,
                  const char *log_path, const char *evt_path, float *bpi, float *implied, int *nblks, int *hit_end) {
   struct deskew_out o = { NULL, nblks, hit_end, bpi, implied };
   return replay_any(opt, parmsets, nparm, tdelta_ns, tstart_ns, nrows, row_base, W, bursts, nbursts, counts, events,
                     exact, exact_free, user, NULL, log_path, evt_path, NULL, 0, &o, 0, INT64_MAX, 0, NULL, NULL, NULL); }

/* ... with the output files made by name as the reference makes them (<out_base>.tap with opt->tap_format, else the numbered
 * <out_base>.NNN.bin files, src/readtape.c:1091-1111) and the end-of-run summary (src/readtape.c:2021-2044) in the log */
int rt_replay_run_named(const struct rt_options *opt, const struct rt_parms *parmsets, int nparm,
                  int64_t tdelta_ns, int64_t tstart_ns, int64_t nrows, int64_t row_base, const int *W,
                  const rtfe_burst *bursts, int64_t nbursts, const uint32_t *counts, const rtfe_event *events,
                  rt_exact_fn exact, rt_exact_free_fn exact_free, void *user,
                  const char *out_base, const char *in_name, const char *log_path, const char *evt_path, int append, struct rt_replay_stats *stats) {
   return replay_any(opt, parmsets, nparm, tdelta_ns, tstart_ns, nrows, row_base, W, bursts, nbursts, counts, events,
                     exact, exact_free, user, NULL, log_path, evt_path, stats, append, NULL, 0, INT64_MAX, 0, out_base, in_name, NULL); }

/* ---------------------------------------------------------------------------------------------------------------------
 * Whirlwind: one chain per tape.  The device detector's state is handed from attempt to attempt (and from chunk to chunk of
 * an attempt); an attempt starts by re-seeding the tracks one per row (src/decoder.c:855-861, after src/decode_ww.c:45 zeroed
 * t_lastpeak) and ends where the host decoder says the clock has stopped (src/decoder.c:892-894) or a block mark was seen.
 * --------------------------------------------------------------------------------------------------------------------- */
static int pred_ww(const struct rt_dec *d, const struct rt_trk *t, double timenow) {
   (void)t;
   return timenow - d->ww.t_lastclkpulseend > d->ww.clkavg.t_bitspaceavg * 1.5f; }             /* WW_CLKSTOP_BITS */

static int ww_readblock_once(void *ctx, int retry) {
   struct rt_replay *rp = (struct rt_replay *)ctx;
   struct rt_dec *d = rp->d;
   const int ntrks = rp->ntrks, W = rp->W[0];
   const size_t sbytes = (size_t)ntrks * rp->ww_track_bytes;
   const int64_t s0 = rp->pos, nrows = rp->nrows, L = rp->ww_chunk_rows;
   int endfile = 0;
   (void)retry;
   ++rp->attempts;
   if (s0 >= nrows) { rt_finish_attempt(d); return 0; }
   int64_t chunk_first = s0;
   memcpy(rp->ww_chunk_state, rp->ww_state, sbytes);
   struct evsrc src; memset(&src, 0, sizeof src);
   int have_chunk = 0;
   int64_t row = s0;
   for (;;) {
      if (!have_chunk) {                                      /* the events of rows [chunk_first, chunk_first + L) */
         if (rp->ww_scan(rp->ww_user, chunk_first, L, s0, rp->ww_chunk_state, rp->ww_chunk_end, rp->ww_counts, rp->ww_events, rp->ww_cap) != 0) {
            ++rp->device_failures; d->results[d->parmset].blktype = RT_BS_ABORTED; rt_finish_attempt(d); return 0; }
         src.stride = rp->ww_event_bytes;
         for (int t = 0; t < ntrks; ++t) { src.list[t] = (const unsigned char *)rp->ww_events + (size_t)t * rp->ww_cap * src.stride; src.n[t] = rp->ww_counts[t]; src.at[t] = 0; }
         src.reset = chunk_first; src.end = chunk_first + L;
         for (int t = 0; t < ntrks; ++t) evsrc_sync(&src, t);
         ++rp->exact_scans;
         have_chunk = 1; }
      /* ---- the next row at which anything can happen ---- */
      int64_t next = nrows;
      if (row < s0 + ntrks) next = row;                       /* the rows on which the tracks are re-seeded, one by one */
      { const int64_t r = evsrc_next_row(&src, ntrks); if (r < next) next = r; }
      if (d->ww.datablock && d->ww.t_lastclkpulseend > 0) {
         const int64_t r = first_row_where(rp, pred_ww, NULL, d->ww.t_lastclkpulseend + d->ww.clkavg.t_bitspaceavg * 1.5f, row, next);
         if (r < next) next = r; }
      if (next >= src.end && src.end < nrows) {               /* nothing more in this chunk: the next one starts from the state behind it */
         chunk_first = src.end;
         memcpy(rp->ww_chunk_state, rp->ww_chunk_end, sbytes);
         have_chunk = 0;
         if (row < chunk_first) row = chunk_first;
         continue; }
      if (next >= nrows) {                                    /* end of data (src/readtape.c:1410-1413; force_end_of_block has no Whirlwind branch) */
         d->timenow = time_of_row(rp, nrows - 1);
         rp->pos = nrows;
         endfile = 1;
         /* the zero-crossing state and the differentiator's last sample survive the -deskew rewind: a pre-pass that read to the end of the data
          * hands the decode the state behind the LAST row (the scan stops at the end of the data; src.end >= nrows here) */
         if (rp->ww_event_bytes == sizeof(rtfe_ww_event)) memcpy(rp->ww_state, rp->ww_chunk_end, sbytes);
         break; }
      row = next;
      rp->cur_row = row;
      d->timenow = time_of_row(rp, row);
      for (int t = 0; t < ntrks; ++t) {                       /* process_sample, src/decoder.c:846-866 */
         struct rt_trk *tk = &d->trk[t];
         if (tk->t_lastpeak == 0) {                            /* first sample of this track in this attempt */
            tk->v_lastpeak = 0;
            tk->t_lastpeak = d->timenow;
            break; }
         while (src.nr[t] == row) {
            if (evsrc_ev(&src, t, src.at[t])->flags & RTFE_EV_FATAL) {
               rp->reference_fatal = 1; d->fatal = 1; rp->fatal_row = row; rp->fatal_trk = t;
               d->results[d->parmset].blktype = RT_BS_ABORTED;
               rt_finish_attempt(d);
               return 0; }
            deliver(rp, &src, t, evsrc_ev(&src, t, src.at[t]), W);
            ++src.at[t]; evsrc_sync(&src, t); } }
      evsrc_skip_before(&src, ntrks, row + 1);
      if (rt_ww_end_due(d)) rt_ww_end_of_block(d);             /* src/decoder.c:892-894 */
      if (d->results[d->parmset].blktype != RT_BS_NONE) { rp->pos = row + 1; break; }
      ++row; }
   if (!endfile) {
      /* where the next attempt starts: the detector's state behind the block's last row */
      const int64_t last = rp->pos - 1;
      if (rp->ww_scan(rp->ww_user, chunk_first, last - chunk_first + 1, s0, rp->ww_chunk_state, rp->ww_state, rp->ww_counts, rp->ww_events, rp->ww_cap) != 0) {
         ++rp->device_failures; d->results[d->parmset].blktype = RT_BS_ABORTED; rt_finish_attempt(d); return 0; } }
   rt_finish_attempt(d);
   return !endfile; }

static int ww_readblock(void *ctx, int retry) {             /* the summary's "samples": as rt_replay_readblock counts them */
   struct rt_replay *rp = (struct rt_replay *)ctx;
   const int64_t from = rp->pos;
   const int more = ww_readblock_once(ctx, retry);
   if (!retry) rp->d->lines_in += (rp->pos - from) + (more ? 0 : 1);
   return more; }

int rt_replay_run_ww(const struct rt_options *opt, const struct rt_parms *parmsets,
                  int64_t tdelta_ns, int64_t tstart_ns, int64_t nrows, int W0, rt_ww_scan_fn scan, void *user, const void *initial_state, int64_t chunk_rows,
                  const char *tap_path, const char *out_base, const char *in_name, const char *log_path, const char *evt_path, struct rt_replay_stats *stats,
                  int deskew, int *delays_out) {
   return rt_replay_run_ww_detector(opt, parmsets, tdelta_ns, tstart_ns, nrows, W0, scan, user, initial_state, sizeof(rtfe_ww_track), chunk_rows,
                                    tap_path, out_base, in_name, log_path, evt_path, stats, deskew, delays_out); }

/* what the -deskew restart does to the device detector's state (src/readtape.c:1676-1716): init_trackpeak_state (src/decoder.c:413-423) clears the
 * window's indices, extremes and countdown and the delay lines - nothing else: the rings, the AGC, the zero detectors' extremes, pending flags and
 * rows and the differentiator's last sample survive the rewind, so the second pass differentiates its first row against the last row the pre-pass
 * read.  The two state kinds of include/rt_frontend.h, told apart by the options that made them. */
static void ww_rewind_state(unsigned char *state, int wide, int ntrks, const struct rt_dec *d, const int *delays) {
   for (int t = 0; t < ntrks; ++t) {
      if (wide) {
         rtfe_ww_dtrack *st = (rtfe_ww_dtrack *)state + t;
         st->left = st->right = st->countdown = 0; st->maxv = st->minv = 0;
         st->v_avg_height = d->trk[t].v_avg_height;
         st->delay = delays[t];
         st->v_raw_row0 = st->v_last_raw; }
      else {
         rtfe_ww_track *st = (rtfe_ww_track *)state + t;
         st->left = st->right = st->maxv = st->minv = st->countdown = 0;
         st->v_avg_height = d->trk[t].v_avg_height;
         st->delay = delays[t]; } } }

int rt_replay_run_ww_detector(const struct rt_options *opt, const struct rt_parms *parmsets,
                  int64_t tdelta_ns, int64_t tstart_ns, int64_t nrows, int W0, rt_ww_scan_fn scan, void *user, const void *initial_state, size_t track_bytes,
                  int64_t chunk_rows, const char *tap_path, const char *out_base, const char *in_name, const char *log_path, const char *evt_path,
                  struct rt_replay_stats *stats, int deskew, int *delays_out) {
   const float sample_deltat = (float)tdelta_ns / 1e9f;
   const int wide = opt->find_zeros || opt->do_differentiate;    /* rtfe_ww_detector_scan: rtfe_ww_dtrack states, rtfe_ww_event records */
   if (track_bytes != (wide ? sizeof(rtfe_ww_dtrack) : sizeof(rtfe_ww_track))) return -4;      /* a state of another detector */
   struct rt_options o = *opt;
   o.multiple_tries = 0;                                       /* "not implemented yet for Whirlwind" (src/readtape.c:1987) */
   struct rt_dec *d = rt_dec_new(&o, sample_deltat, tdelta_ns);
   if (!d) return -1;
   if (parmsets) { memset(d->parmsets, 0, sizeof d->parmsets); memcpy(d->parmsets, parmsets, sizeof(struct rt_parms)); }
   else for (int i = 1; i < RT_MAXPARMSETS; ++i) d->parmsets[i].active = 0;
   if (out_base) snprintf(d->outbase, sizeof d->outbase, "%s", out_base);
   else if (tap_path) d->tapf = fopen(tap_path, "wb");
   if (log_path) d->logf = fopen(log_path, "w");
   struct rt_replay rp; memset(&rp, 0, sizeof rp);
   rp.d = d; rp.ntrks = o.ntrks; rp.nparm = 1; rp.W[0] = W0;
   rp.nrows = nrows; rp.tstart_ns = tstart_ns; rp.tdelta_ns = tdelta_ns; rp.stop_row = INT64_MAX;
   rp.ww_scan = scan; rp.ww_user = user;
   rp.find_zeros = o.find_zeros;
   rp.ww_track_bytes = track_bytes; rp.ww_event_bytes = wide ? sizeof(rtfe_ww_event) : sizeof(rtfe_event);
   rp.ww_chunk_rows = chunk_rows > 64 ? chunk_rows : 64;
   rp.ww_cap = (uint32_t)rp.ww_chunk_rows;                     /* (no more events than rows) */
   const size_t sbytes = (size_t)o.ntrks * track_bytes;
   rp.ww_state = (unsigned char *)malloc(3 * sbytes); rp.ww_chunk_state = rp.ww_state + sbytes; rp.ww_chunk_end = rp.ww_state + 2 * sbytes;
   memcpy(rp.ww_state, initial_state, sbytes);
   rp.ww_events = (rtfe_event *)malloc((size_t)o.ntrks * rp.ww_cap * rp.ww_event_bytes);
   rp.ww_counts = (uint32_t *)calloc((size_t)o.ntrks, sizeof(uint32_t));
   if (evt_path) {
      rp.evtf = fopen(evt_path, "wb");
      if (rp.evtf) { d->on_transition = dump_transition; d->on_attempt = dump_attempt; d->user = &rp; } }
   const double wall0 = (double)time(NULL);
   struct rt_reader rd = { ww_readblock, rt_replay_save_pos, rt_replay_restore_pos, &rp };
   int prepass_failed = 0;
   const int peaks = peak_attach(d);
   if (deskew) {
      /* -deskew (src/readtape.c:1676-1716): the first blocks are read once to learn the heads' skew and the pulse heights; then the
       * windows and the delay lines are cleared (init_trackpeak_state) - NOT the rings, the AGC or the decoder's track state -
       * and the tape is read again from its first row, every track behind its delay */
      int delays[RT_MAXTRKS] = { 0 }, hit_end = 0;
      rt_replay_save_pos(&rp);
      const int nblks = rt_deskew_prepass(d, &rd, delays, &hit_end);
      rt_replay_restore_pos(&rp);
      if (nblks < 0 || rp.device_failures || rp.reference_fatal) prepass_failed = 1;
      else {
         if (peaks) { peak_keep(d, 1); memset(&d->peakstat, 0, sizeof d->peakstat); }      /* (a decode that records nothing reports nothing: no stale counts) */
         ww_rewind_state(rp.ww_state, wide, o.ntrks, d, delays);
         if (delays_out) memcpy(delays_out, delays, sizeof(int) * (size_t)o.ntrks); } }
   struct rt_textfile *text = prepass_failed ? NULL : text_attach(d);
   const int ok = prepass_failed ? 0 : rt_process_blocks(d, &rd, 0x7fffffff);
   if (text) { d->text = NULL; d->text_record = NULL; d->text_tapemark = NULL; rt_text_close(text, 1); }
   if (in_name) rt_write_summary(d, in_name, difftime(time(NULL), (time_t)wall0));
   if (peaks && !prepass_failed) peak_report(d);
   if (stats) {
      memset(stats, 0, sizeof *stats);
      stats->attempts = rp.attempts; stats->exact_scans = rp.exact_scans; stats->events_delivered = rp.events_delivered; stats->agc_mismatches = rp.agc_mismatches;
      stats->blocks = d->numblks; stats->tapemarks = d->numtapemarks; stats->blocks_with_errors = d->numblks_err;
      stats->blocks_with_warnings = d->numblks_warn; stats->blocks_unusable = d->numblks_unusable; stats->all_ok = ok;
      stats->data_bytes = d->numdatabytes; stats->device_failures = rp.device_failures;
      stats->reference_fatal = rp.reference_fatal; stats->fatal_row = rp.fatal_row; stats->fatal_trk = rp.fatal_trk; }
   if (d->tapf) fclose(d->tapf);
   if (d->logf) fclose(d->logf);
   if (rp.evtf) fclose(rp.evtf);
   free(rp.ww_state); free(rp.ww_events); free(rp.ww_counts);
   rt_dec_free(d);
   return (prepass_failed && !rp.device_failures && !rp.reference_fatal) ? -2 : 0; }

/* ---------------------------------------------------------------------------------------------------------------------
 * The finisher: ONE context for the whole tape.  It takes this thread's requests (rt_replay_set_text, rt_driver_set_run, rt_replay_set_peakstats) as the
 * resident decode's run does, is given the fragments' journals in tape order, and ends with what ends a resident run: end_of_blocks, the summary, the
 * peak statistics' report.  All its calls are made on the thread that made it.
 * --------------------------------------------------------------------------------------------------------------------- */
struct rt_finisher {
   struct rt_dec *d; struct rt_textfile *text; struct rt_peakbins *bins;
   int peaks, blklimit, limited, has_in; char in_name[1024];
   int64_t lines_base, prev_final_abs, prev_end_counted, fragments; double wall0, seconds;
   int all_ok; struct journal_work work; int64_t device_failures, reference_fatal, fatal_row, fatal_trk;
   int32_t tried[RT_MAXPARMSETS], chosen[RT_MAXPARMSETS], goodmultiple; };

static double mono_now(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec; }

struct rt_finisher *rt_journal_finisher_new(const struct rt_options *opt, const struct rt_parms *parmsets, int nparm, int64_t tdelta_ns,
                  const char *tap_path, const char *out_base, const char *in_name, const char *log_path, int append, struct rt_peakbins *bins) {
   struct rt_finisher *f = (struct rt_finisher *)calloc(1, sizeof *f);
   if (!f) return NULL;
   struct rt_dec *d = rt_dec_new(opt, (float)tdelta_ns / 1e9f, tdelta_ns);
   if (!d) { free(f); return NULL; }
   f->d = d; f->bins = bins; f->all_ok = 1;
   if (parmsets) {
      memset(d->parmsets, 0, sizeof d->parmsets);
      memcpy(d->parmsets, parmsets, sizeof(struct rt_parms) * (size_t)nparm); }
   else for (int i = nparm; i < RT_MAXPARMSETS; ++i) d->parmsets[i].active = 0;
   if (out_base) snprintf(d->outbase, sizeof d->outbase, "%s", out_base);
   else if (tap_path) d->tapf = fopen(tap_path, "wb");
   if (log_path) d->logf = fopen(log_path, append ? "a" : "w");
   if (in_name) { snprintf(f->in_name, sizeof f->in_name, "%s", in_name); f->has_in = 1; }
   f->wall0 = (double)time(NULL);
   f->peaks = bins ? peak_attach(d) : 0;
   f->text = text_attach(d);
   f->blklimit = rt_driver_take_run(d, 0x7fffffff);
   return f; }

static void finisher_learn_bins(struct rt_finisher *f, float left, float bw) {
   if (!f->d->peakstat.initialized) rt_peakstat_start(f->d, left, bw); }

/* a fragment's histogram (as it was when the fragment ended, or at the record the block limit falls on) into the tape's: integer sums, in any order */
static void finisher_add_peaks(struct rt_finisher *f, const struct rt_journal *j, const struct peak_counts *p) {
   struct rt_dec *d = f->d;
   struct rt_peakbins *B = f->bins;
   if (!B || !(p->initialized || p->nraw > 0)) return;
   int64_t nraw = p->nraw < j->raw_cap ? p->nraw : j->raw_cap;
   pthread_mutex_lock(&B->mu);
   if (!B->have && nraw > 0) { rt_peakstat_bins(d->opt.mode, j->raw[0].bitspacing, &B->leftbin, &B->binwidth); B->have = 1; }      /* (in tape order: the tape's first) */
   const int have = B->have; const float left = B->leftbin, bw = B->binwidth;
   pthread_mutex_unlock(&B->mu);
   if (!have) return;
   finisher_learn_bins(f, left, bw);
   for (int64_t i = 0; i < nraw; ++i) if (j->raw[i].trk >= 0 && j->raw[i].trk < RT_MAXTRKS) rt_peakstat_count(d, j->raw[i].peaktime, j->raw[i].trk);
   if (p->initialized)
      for (int t = 0; t < RT_MAXTRKS; ++t) {
         d->peakstat.trksums[t] += p->trksums[t];
         for (int b = 0; b < RT_PEAKSTAT_BUCKETS; ++b) d->peakstat.counts[t][b] += p->counts[t][b]; } }

/* The next fragment's journal, in tape order.  Returns 0, 1 once the block limit is reached (the journals behind it are not wanted), -1 for a journal
 * that is not whole. */
int rt_journal_finish(struct rt_finisher *f, struct rt_journal *j) {
   if (!f || !j || !j->done || j->failed) return -1;
   if (f->limited) return 1;
   const double t0 = mono_now();
   struct rt_dec *d = f->d;
   /* lines_in ("samples were processed"): the fragment counted from its own start, the resident decode's attempt would have started where the fragment
    * in front ended; and every fragment but the tape's last counted the + 1 of an end of the data */
   const int64_t base = f->lines_base + (j->start_abs - f->prev_final_abs) - f->prev_end_counted;
   size_t at = 0;
   int rc = 0;
   const struct peak_counts *limit_peak = NULL;
   struct peak_counts snap;
   struct jrec r;
   if (d->numblks >= f->blklimit) { f->limited = 1; rc = 1; }      /* (a limit of 0) */
   while (!rc && at < j->len) {
      if (j->len - at < sizeof r) { rc = -1; break; }
      memcpy(&r, j->buf + at, sizeof r); at += sizeof r;
      const size_t words = (size_t)(r.ndata < 0 ? 0 : r.ndata) + (size_t)(r.nfaked < 0 ? 0 : r.nfaked);
      if (r.magic != JREC_MAGIC || r.ndata < 0 || r.ndata > RT_MAXBLOCK || (r.nfaked != 0 && r.nfaked != r.ndata) || r.parmset < 0 || r.parmset >= RT_MAXPARMSETS
          || j->len - at < words * sizeof(uint16_t) + (r.has_snap ? sizeof snap : 0)) { rc = -1; break; }
      memcpy(d->data, j->buf + at, sizeof(uint16_t) * (size_t)r.ndata); at += sizeof(uint16_t) * (size_t)r.ndata;
      if (r.nfaked) { memcpy(d->data_faked, j->buf + at, sizeof(uint16_t) * (size_t)r.nfaked); at += sizeof(uint16_t) * (size_t)r.nfaked; }
      if (r.has_snap) { memcpy(&snap, j->buf + at, sizeof snap); at += sizeof snap; }
      d->parmset = r.parmset; d->tries = r.tries; d->results[r.parmset] = r.res;
      d->timenow = r.timenow; d->t_blockstart = r.t_blockstart;
      d->lines_in = base + r.lines_in;
      d->numblks_goodmultiple = f->goodmultiple + r.goodmultiple;
      for (int i = 0; i < RT_MAXPARMSETS; ++i) { d->parmsets[i].tried = f->tried[i] + r.tried[i]; d->parmsets[i].chosen = f->chosen[i] + r.chosen[i]; }
      switch ((enum rt_bstate)r.blktype) {
      case RT_BS_TAPEMARK: rt_got_tapemark(d); break;
      case RT_BS_BLOCK:    rt_got_datablock(d, 0); break;
      case RT_BS_BADBLOCK: rt_got_datablock(d, 1); break;
      default: rc = -1; break; }
      if (!rc && d->numblks >= f->blklimit) {                    /* as rt_process_blocks' loop ends: behind the block that reaches the limit */
         f->limited = 1; rc = 1;
         f->all_ok = f->all_ok && r.all_clean;
         f->work.attempts += r.work.attempts; f->work.exact_scans += r.work.exact_scans; f->work.chained += r.work.chained;
         f->work.events_delivered += r.work.events_delivered; f->work.agc_mismatches += r.work.agc_mismatches;
         if (r.has_snap) limit_peak = &snap; } }
   if (rc == 0) {                                               /* the whole fragment */
      d->timenow = j->timenow;
      d->lines_in = base + j->lines_in;
      f->lines_base = d->lines_in; f->prev_final_abs = j->final_abs; f->prev_end_counted = j->end_counted;
      f->goodmultiple += j->goodmultiple; d->numblks_goodmultiple = f->goodmultiple;
      for (int i = 0; i < RT_MAXPARMSETS; ++i) { f->tried[i] += j->tried[i]; f->chosen[i] += j->chosen[i]; d->parmsets[i].tried = f->tried[i]; d->parmsets[i].chosen = f->chosen[i]; }
      f->all_ok = f->all_ok && j->all_clean;
      /* the replay's own counters are the work the fragments did (each closes with an attempt that finds nothing, each starts on a zone's first row) */
      f->work.attempts += j->stats.attempts; f->work.exact_scans += j->stats.exact_scans;
      f->work.chained += j->stats.chained;
      f->work.events_delivered += j->stats.events_delivered; f->work.agc_mismatches += j->stats.agc_mismatches;
      finisher_add_peaks(f, j, &j->peak); }
   else if (rc == 1 && limit_peak) finisher_add_peaks(f, j, limit_peak);
   if (rc >= 0) {
      f->device_failures += j->stats.device_failures;
      if (j->stats.reference_fatal && !f->reference_fatal) { f->reference_fatal = j->stats.reference_fatal; f->fatal_row = j->stats.fatal_row; f->fatal_trk = j->stats.fatal_trk; }
      ++f->fragments; }
   f->seconds += mono_now() - t0;
   return rc; }

/* What ends a run: the end of the output file(s), the summary, the statistics' report.  Fills *stats as a resident replay would (the replay's own counters
 * are the fragments' sums), *seconds = the time spent in rt_journal_finish and here.  Frees the finisher. */
int rt_journal_finisher_end(struct rt_finisher *f, struct rt_replay_stats *stats, double *seconds) {
   if (!f) return -1;
   const double t0 = mono_now();
   struct rt_dec *d = f->d;
   if (!f->limited) d->lines_in = f->lines_base;
   rt_end_of_blocks(d, f->blklimit);
   if (f->text) { d->text = NULL; d->text_record = NULL; d->text_tapemark = NULL; rt_text_close(f->text, 1); }
   if (f->has_in) rt_write_summary(d, f->in_name, difftime(time(NULL), (time_t)f->wall0));
   if (f->peaks) {
      if (f->bins && !d->peakstat.initialized) {                /* (no transition anywhere: the report is the resident decode's of an untouched histogram) */
         memset(&d->peakstat, 0, sizeof d->peakstat); }
      peak_report(d); }
   if (stats) {
      memset(stats, 0, sizeof *stats);
      stats->attempts = f->work.attempts; stats->exact_scans = f->work.exact_scans; stats->chained = f->work.chained;
      stats->events_delivered = f->work.events_delivered; stats->agc_mismatches = f->work.agc_mismatches;
      stats->blocks = d->numblks; stats->tapemarks = d->numtapemarks; stats->blocks_with_errors = d->numblks_err;
      stats->blocks_with_warnings = d->numblks_warn; stats->blocks_unusable = d->numblks_unusable; stats->all_ok = f->all_ok;
      stats->data_bytes = d->numdatabytes; stats->device_failures = f->device_failures;
      stats->reference_fatal = f->reference_fatal; stats->fatal_row = f->fatal_row; stats->fatal_trk = f->fatal_trk; }
   if (d->tapf) fclose(d->tapf);
   if (d->logf) fclose(d->logf);
   f->seconds += mono_now() - t0;
   if (seconds) *seconds = f->seconds;
   rt_dec_free(d);
   free(f);
   return 0; }
