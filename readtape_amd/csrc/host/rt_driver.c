/* rt_driver.c — block retry / best-decoding selection and the SIMH .tap writer.
 * Restates the block loop of src/readtape.c:1720-1882 and the writers of src/readtape.c:1076-1082,
 * 1160-1176, 1212-1313, 1885 over an abstract block reader, so the same decisions are taken whether
 * the attempts are re-read one at a time (scalar path) or looked up in a batched parmset sweep. */
#include "rt_decode.h"

#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static void rlog(struct rt_dec *d, const char *fmt, ...) {
   if (!d->logf) return;
   va_list ap; va_start(ap, fmt); vfprintf(d->logf, fmt, ap); va_end(ap); }

static void output_tap_marker(struct rt_dec *d, uint32_t num) {   /* src/readtape.c:1076-1082 */
   for (int i = 0; i < 4; ++i) {
      unsigned char lsb = num & 0xff;
      if (d->tapf) fwrite(&lsb, 1, 1, d->tapf);
      num >>= 8; }
   d->numoutbytes += 4; }

/* 1234567 -> "1,234,567": how the reference prints byte and sample counts (src/readtape.c:707-718) */
static const char *commas(long long n, char buf[32]) {
   char raw[24];
   const int len = snprintf(raw, sizeof raw, "%lld", n);
   int o = 0;
   for (int i = 0; i < len; ++i) { buf[o++] = raw[i]; if ((len - 1 - i) % 3 == 0 && i != len - 1) buf[o++] = ','; }
   buf[o] = 0;
   return buf; }

/* ---- output files (src/readtape.c:1084-1111).  Two ways to use the writers: the caller opens d->tapf itself (one .tap, nothing
 * logged about it), or it sets d->outbase and the files are made here, by the reference's names and with its log lines ---- */
void rt_close_output(struct rt_dec *d) {
   if (!d->tapf) return;
   fclose(d->tapf);
   d->tapf = NULL;
   if (!d->outbase[0]) return;
   char cb[32];
   rlog(d, "%s was closed at time %.8lf after %s data bytes were extracted from %d blocks\n", d->outname, d->timenow, commas(d->numfilebytes, cb), d->numfileblks); }

/* labelled != NULL: the name an HDR1 label gave the file (src/readtape.c:1094-1097) */
static void open_output(struct rt_dec *d, const char *labelled) {
   if (!d->outbase[0]) return;
   if (d->tapf) rt_close_output(d);
   if (labelled) snprintf(d->outname, sizeof d->outname, "%s.bin", labelled);
   else if (d->opt.tap_format) snprintf(d->outname, sizeof d->outname, "%s.tap", d->outbase);
   else snprintf(d->outname, sizeof d->outname, "%s.%03d.bin", d->outbase, d->numfiles + 1);
   rlog(d, "creating file \"%s\"\n", d->outname);
   d->tapf = fopen(d->outname, "wb");
   ++d->numfiles;
   d->numfilebytes = 0;
   d->numfileblks = 0;
   if (d->data_start_time == 0) d->data_start_time = d->timenow; }

void rt_tap_end(struct rt_dec *d) {   /* src/readtape.c:1885-1887: the end-of-medium marker only if the file was ever created */
   const int created = d->outbase[0] ? d->tapf != NULL : (d->tapf && d->numoutbytes > 0);
   if (d->opt.tap_format && created && !d->no_tap_end) output_tap_marker(d, 0xffffffffu);
   if (d->outbase[0]) rt_close_output(d); }

static void text_file_logged(struct rt_dec *d) {   /* the text file is made by what is first written to it (src/textfile.c:198) */
   if (!d->text_logged && d->text_name) rlog(d, "creating file \"%s\"\n", d->text_name);
   d->text_logged = 1; }

void rt_got_tapemark(struct rt_dec *d) {   /* src/readtape.c:1160-1176 */
   ++d->numtapemarks;
   rlog(d, "  tapemark at time %.8lf, tap offset %lld, %d blocks written so far\n", d->timenow, d->numoutbytes, d->numblks);
   if (d->text_tapemark) { text_file_logged(d); d->text_tapemark(d->text, d->timenow); }
   if (d->opt.tap_format) {
      if (!d->tapf) open_output(d, NULL);
      output_tap_marker(d, 0x00000000); }
   else if (!d->hdr1_seen) rt_close_output(d);      /* plain data files: a tapemark ends the file, unless an HDR1 label named it (EOF1 will) */
   d->hdr1_seen = 0; }

static const char *format_block_errors(struct rt_dec *d, struct rt_results *result, char *buf) {   /* src/readtape.c:1179-1209 */
   char *p = buf;
   if (result->errcount > 0) {
      p += sprintf(p, "%d err%s", result->errcount, result->errcount > 1 ? "s" : "");
      if (result->track_mismatch) p += sprintf(p, ", %d bit track mismatch", result->track_mismatch);
      if (result->vparity_errs) p += sprintf(p, ", %d parity", result->vparity_errs);
      if (result->crc_errs) p += sprintf(p, ", %d CRC", result->crc_errs);
      if (result->lrc_errs) p += sprintf(p, ", 1 LRC");
      if (result->ecc_errs) p += sprintf(p, ", %d ECC", result->ecc_errs);
      if (result->ww_bad_length) p += sprintf(p, ", bad length");
      if (result->ww_speed_err) p += sprintf(p, ", bad speed"); }
   else p += sprintf(p, "ok");
   if (result->warncount > 0) {
      p += sprintf(p, ", %d warning%s", result->warncount, result->warncount > 1 ? "s" : "");
      if (d->opt.mode == RT_NRZI && result->corrected_bits > 0) {
         int trkcount = 0; uint16_t tracks = result->faked_tracks;
         for (; tracks; ++trkcount) tracks &= tracks - 1;
         p += sprintf(p, ", %d bits corrected on %d trks", result->corrected_bits, trkcount); }
      if (result->gcr_bad_dgroups) p += sprintf(p, ", %d bad dgroups", result->gcr_bad_dgroups);
      if (result->corrected_bits > 0) p += sprintf(p, ", %d corrected bits", result->corrected_bits);
      if (d->opt.mode == RT_PE) {
         int length = result->minbits, nbits = 0, ntrk = 0; uint16_t faked = 0;
         for (int i = 0; i < length; ++i) { uint16_t v = d->data_faked[i]; faked |= v; for (; v; ++nbits) v &= v - 1; }
         for (; faked; ++ntrk) faked &= faked - 1;
         if (nbits > 0) p += sprintf(p, ", %d faked bits on %d trks", nbits, ntrk); }
      if (result->ww_leading_clock) p += sprintf(p, ", leading clk");
      if (result->ww_missing_onebit) p += sprintf(p, ", missing 1-bit");
      if (result->ww_missing_clock) p += sprintf(p, ", missing clk"); }
   return buf; }

/* the block's line in the verbose text file (src/textfile.c:246-249) and its data without the parity bit */
static void text_datablock(struct rt_dec *d, struct rt_results *result, int length) {
   char head[480], errs[400];
   unsigned char *bytes = (unsigned char *)malloc((size_t)length + 1);
   if (!bytes) return;
   for (int i = 0; i < length; ++i) bytes[i] = (unsigned char)(d->data[i] >> 1);
   snprintf(head, sizeof head, "block %d: %d bytes at time %.8lf, %s", d->numblks + 1, length, d->timenow, format_block_errors(d, result, errs));
   text_file_logged(d);
   d->text_record(d->text, bytes, length, result->errcount, result->warncount, head);
   free(bytes); }

/* ---- IBM standard tape labels (src/ibmlabels.c:118-168): 80-byte blocks of EBCDIC text that start VOL1, HDR1/EOF1/EOV1 or HDR2/EOF2/EOV2.
 * They are logged; without -tap they are not data (not written, not counted), HDR1 names the data file that follows
 * <outbase>-NNN-<dataset id>.bin and EOF1 closes it.  The table is the label reader's own (unmapped codes are '?', src/ibmlabels.c:71-87),
 * not the text dump's. ---- */
static unsigned char label_ascii(uint16_t w) {
   static const char rows4_7[4][17] = { " ?????????[.<(+|", "&?????????" "!$*);^", "-/????????|,%_>?", "?????????`:#|'=\"" };
   const unsigned c = (w >> 1) & 0xff, hi = c >> 4, lo = c & 15;
   if (c == 0x00 || c == 0xff) return ' ';
   if (hi >= 4 && hi <= 7) return (unsigned char)rows4_7[hi - 4][lo];
   if (hi >= 8 && hi <= 0xa) {                                  /* lower case: a-i, j-r, ~ s-z */
      if (hi == 0xa) return lo == 1 ? '~' : (lo >= 2 && lo <= 9) ? (unsigned char)('s' + lo - 2) : '?';
      return (lo >= 1 && lo <= 9) ? (unsigned char)((hi == 8 ? 'a' : 'j') + lo - 1) : '?'; }
   if (hi >= 0xc && hi <= 0xe) {                                /* upper case, with { } \ in column 0 */
      if (lo == 0) return (unsigned char)"{}\\"[hi - 0xc];
      if (hi == 0xe) return (lo >= 2 && lo <= 9) ? (unsigned char)('S' + lo - 2) : '?';
      return lo <= 9 ? (unsigned char)((hi == 0xc ? 'A' : 'J') + lo - 1) : '?'; }
   if (hi == 0xf) return lo <= 9 ? (unsigned char)('0' + lo) : '?';
   return '?'; }

/* a field of the label as a string without its trailing blanks */
static const char *label_field(const unsigned char *text, int at, int len, char *buf) {
   memcpy(buf, text + at, (size_t)len);
   while (len > 0 && buf[len - 1] == ' ') --len;
   buf[len] = 0;
   return buf; }

static int absorb_label(struct rt_dec *d, const struct rt_results *result) {
   if (result->minbits != 80) return 0;
   unsigned char t[81];
   for (int i = 0; i < 4; ++i) t[i] = label_ascii(d->data[i]);
   const int seq = t[3] == '1' ? 1 : t[3] == '2' ? 2 : 0;
   const int vol = !memcmp(t, "VOL", 3), hdr = !memcmp(t, "HDR", 3), eof = !memcmp(t, "EOF", 3), eov = !memcmp(t, "EOV", 3);
   if (!seq || !(hdr || eof || eov || (vol && seq == 1))) return 0;
   for (int i = 4; i < 80; ++i) t[i] = label_ascii(d->data[i]);
   t[80] = 0;
   char a[20], b[20], c[20];
   if (vol) rlog(d, "*** tape label %.4s, serno \"%s\", owner \"%s\"\n", t, label_field(t, 4, 6, a), label_field(t, 41, 10, b));
   else if (seq == 1) {
      rlog(d, "*** tape label %.4s, dsid \"%s\", serno \"%s\", created%s\n", t, label_field(t, 4, 17, a), label_field(t, 21, 6, b), label_field(t, 41, 6, c));
      rlog(d, "    volume %s, dataset %s\n", label_field(t, 27, 4, a), label_field(t, 31, 4, b));
      if (eof) rlog(d, "    block count %.6s, system %s\n", t + 54, label_field(t, 60, 13, a)); }
   else {
      rlog(d, "*** tape label %.4s, RECFM=%.1s%.1s, BLKSIZE=%s, LRECL=%s\n", t, t + 4, t + 38, label_field(t, 5, 5, a), label_field(t, 10, 5, b));
      rlog(d, "    job: \"%s\"\n", label_field(t, 17, 17, a)); }
   if (result->errcount) rlog(d, "--> %d errors\n", result->errcount);
   if (seq == 1 && hdr) {
      if (!d->opt.tap_format && d->outbase[0]) {
         char name[1080];
         snprintf(name, sizeof name, "%.1024s-%03d-%s", d->outbase, d->numfiles + 1, label_field(t, 4, 17, a));
         open_output(d, name); }
      d->hdr1_seen = 1; }
   if (seq == 1 && eof && !d->opt.tap_format && d->outbase[0]) rt_close_output(d);
   return 1; }

void rt_got_datablock(struct rt_dec *d, int badblock) {   /* src/readtape.c:1212-1313 */
   struct rt_results *result = &d->results[d->parmset];
   int length = result->minbits;
   const int labelled = !badblock && d->labels && absorb_label(d, result);
   if (length > 0 && (d->opt.tap_format || !labelled)) {
      if (badblock) {
         ++d->numblks_unusable;
         rlog(d, "ERROR: unusable block, ");
         if (result->track_mismatch) rlog(d, "tracks mismatched with lengths %d to %d", result->minbits, result->maxbits);
         else rlog(d, "unknown reason");
         rlog(d, ", %d tries, parmset %d, at time %.8lf\n", d->tries, d->parmset, d->timenow); }
      else {
         uint32_t errflag = result->errcount ? 0x80000000u : 0;
         d->last_block_time = d->timenow;
         if (!d->tapf) open_output(d, NULL);
         if (d->opt.tap_format) output_tap_marker(d, (uint32_t)length | errflag);
         for (int i = 0; i < length; ++i) {
            unsigned char b = (unsigned char)(d->data[i] >> 1);
            if (d->opt.add_parity) b |= (d->data[i] & 1) << (d->opt.ntrks - 1);
            if (d->tapf) fwrite(&b, 1, 1, d->tapf); }
         if (d->opt.tap_format) {
            unsigned char zero = 0;
            if (length & 1) {
               if (d->tapf) fwrite(&zero, 1, 1, d->tapf);
               d->numoutbytes += 1; }
            output_tap_marker(d, (uint32_t)length | errflag); }
         if (d->text_record) text_datablock(d, result, length);
         if (result->errcount != 0) ++d->numblks_err;
         if (result->warncount != 0) ++d->numblks_warn;
         if (d->opt.verbose || d->numblks == 0 || result->errcount > 0 || result->warncount > 0) {
            char buf[400];
            rlog(d, "wrote block %3d, %4d bytes, %d %s, parmset %d, ", d->numblks + 1, length, d->tries, d->tries > 1 ? "tries" : "try", d->parmset);
            if (result->alltrk_min_agc_gain == FLT_MAX) rlog(d, "max AGC %.2f, ", result->alltrk_max_agc_gain);
            else rlog(d, "AGC %.2f-%.2f, ", result->alltrk_min_agc_gain, result->alltrk_max_agc_gain);
            rlog(d, "%s", format_block_errors(d, result, buf));
            rlog(d, ", avg speed %.2f IPS at time %.8lf", 1 / (result->avg_bit_spacing * d->opt.bpi), d->timenow);
            rlog(d, ", tap offset %lld\n", d->numoutbytes); }
         if (result->track_mismatch) ++d->numblks_trksmismatched;
         if (result->missed_midbits > 0) {
            ++d->numblks_midbiterrs;
            rlog(d, "   WARNING: %d bits were before the midbit using parmset %d for block %d at %.8lf\n",
                 result->missed_midbits, d->parmset, d->numblks + 1, d->timenow); }
         if (result->corrected_bits > 0) ++d->numblks_corrected;
         d->numfilebytes += length;
         d->numoutbytes += length;
         d->numdatabytes += length;
         ++d->numfileblks;
         ++d->numblks; } } }

/* the end-of-run report (src/readtape.c:2021-2044) */
void rt_write_summary(struct rt_dec *d, const char *infilename, double elapsed) {
   char cb[32];
   rlog(d, "\n");
   rlog(d, "summary for file \"%s\":\n", infilename);
   rlog(d, "  %s samples were processed in %.0lf seconds (%.3lf seconds/block)\n", commas(d->lines_in, cb), elapsed, d->numblks == 0 ? 0 : elapsed / d->numblks);
   rlog(d, "  created %d output file%s with a total of %s bytes\n", d->numfiles, d->numfiles != 1 ? "s" : "", commas(d->numoutbytes, cb));
   rlog(d, "  decoded %d tape marks and %d blocks with %s bytes from %.2lf seconds of tape data\n",
        d->numtapemarks, d->numblks, commas(d->numdatabytes, cb), d->timenow - d->data_start_time);
   if (d->last_block_time) rlog(d, "  the last block written was %.8lf seconds into the tape\n", d->last_block_time);
   rlog(d, "  %d block%s had errors, %d had warnings", d->numblks_err, d->numblks_err != 1 ? "s" : "", d->numblks_warn);
   if (d->opt.mode != RT_WW) rlog(d, ", %d had mismatched tracks, %d had bits corrected", d->numblks_trksmismatched, d->numblks_corrected);
   if (d->opt.mode == RT_NRZI) rlog(d, ", %d had midbit timing errors", d->numblks_midbiterrs);
   rlog(d, "\n");
   if (d->opt.mode == RT_WW && d->num_flux_polarity_changes > 0)
      rlog(d, "  the flux polarity changed %d time%s during decoding\n", d->num_flux_polarity_changes, d->num_flux_polarity_changes > 1 ? "s" : "");
   if (d->numblks_unusable > 0) rlog(d, "  %d blocks were unusable and were not written\n", d->numblks_unusable);
   if (!d->opt.multiple_tries) return;
   rlog(d, "  %d good blocks had to try more than one parmset\n", d->numblks_goodmultiple);
   for (int i = 0; i < RT_MAXPARMSETS; ++i)
      if (d->parmsets[i].tried > 0)
         rlog(d, "  parmset %d was tried %4d times and used %4d times, or %5.1f%%\n", i, d->parmsets[i].tried, d->parmsets[i].chosen,
              100. * d->parmsets[i].chosen / d->parmsets[i].tried); }

/* ---- one block, possibly many attempts (src/readtape.c:1720-1882) ----
 * An attempt is FINAL when nothing could improve on it: a tapemark, noise (the reference skips noise at once, SKIP_NOISE), or
 * a block without errors or warnings.  Otherwise, with -m, the next parameter set that has not been tried on this block gets
 * its turn; when none is left the attempts are RANKED and the best one is (if it was not the last one run) decoded again so
 * that the bit matrix holds its data. */
static int attempt_is_final(const struct rt_results *a) {
   return a->blktype == RT_BS_TAPEMARK || a->blktype == RT_BS_NOISE
          || (a->blktype == RT_BS_BLOCK && a->errcount == 0 && a->warncount == 0); }

/* the parameter set to try next: the first active, untried one behind the current one (cyclically), or -1 */
static int untried_parmset(const struct rt_dec *d) {
   for (int step = 1; step < RT_MAXPARMSETS; ++step) {
      const int p = (d->parmset + step) % RT_MAXPARMSETS;
      if (d->parmsets[p].active != 0 && d->results[p].blktype == RT_BS_NONE) return p; }
   return -1; }

/* rank of an attempt among the imperfect ones, smaller is better (src/readtape.c:1805-1845): error-free blocks by their
 * warnings, then blocks by their errors, then ragged blocks by their raggedness, then noise; the earlier parameter set wins
 * a tie.  Returns 0 for an attempt that cannot be chosen. */
static int attempt_rank(const struct rt_results *a, int *tier, int *badness) {
   switch (a->blktype) {
   case RT_BS_BLOCK:    *tier = a->errcount == 0 ? 0 : 1; *badness = a->errcount == 0 ? a->warncount : a->errcount; return 1;
   case RT_BS_BADBLOCK: *tier = 2; *badness = a->track_mismatch; return 1;
   case RT_BS_NOISE:    *tier = 3; *badness = 0; return 1;
   default: return 0; } }

static int best_attempt(const struct rt_dec *d, int *tier_out) {
   int best = -1, best_tier = INT_MAX, best_badness = INT_MAX;
   for (int p = 0; p < RT_MAXPARMSETS; ++p) {
      int tier, badness;
      if (!attempt_rank(&d->results[p], &tier, &badness)) continue;
      if (badness == INT_MAX) continue;                         /* (the reference's "< INT_MAX" searches cannot pick such a value either) */
      if (tier < best_tier || (tier == best_tier && badness < best_badness)) { best = p; best_tier = tier; best_badness = badness; } }
   *tier_out = best_tier;
   return best; }

static __thread struct { int set, labels, blklimit; } g_run_request;
void rt_driver_set_run(int labels, int blklimit) {
   g_run_request.set = 1; g_run_request.labels = labels; g_run_request.blklimit = blklimit; }

static void end_of_blocks(struct rt_dec *d, int blklimit) {      /* src/readtape.c:1884-1887 */
   if (d->numblks >= blklimit) rlog(d, "\n***blklimit=%d reached\n", blklimit);
   rt_tap_end(d); }
void rt_end_of_blocks(struct rt_dec *d, int blklimit) { end_of_blocks(d, blklimit); }

int rt_driver_take_run(struct rt_dec *d, int blklimit) {
   if (g_run_request.set) {
      g_run_request.set = 0;
      d->labels = g_run_request.labels;
      if (g_run_request.blklimit >= 0 && g_run_request.blklimit < blklimit) blklimit = g_run_request.blklimit; }
   return blklimit; }

int rt_process_blocks(struct rt_dec *d, struct rt_reader *r, int blklimit) {
   int out_of_data = 0;
   d->run_all_clean = 1;                                          /* (in the context, where on_block can read it) */
   blklimit = rt_driver_take_run(d, blklimit);
   const int ww = d->opt.mode == RT_WW;
   d->interblock_counter = 0;
   if (ww && !d->ww_prepassed) rt_init_trackstate(d);             /* Whirlwind: once per tape - blocks may be one bit apart (src/readtape.c:1674); a -deskew pre-pass has done it */
   while (!out_of_data && d->numblks < blklimit) {
      rt_init_blockstate(d);
      d->parmset = 0;
      d->tries = 0;
      r->save_pos(r->ctx);
      int decoded_last, final = 0;
      for (;;) {                                                  /* attempts */
         decoded_last = d->parmset;
         if (ww) rt_ww_init_blockstate(d); else rt_init_trackstate(d);
         if (ww && d->ww.blockmark_queued) {                      /* the block mark seen while the last block's end was being noticed */
            rt_ww_blockmark(d);
            d->t_blockstart = d->timenow - d->ww.clkavg.t_bitspaceavg; }
         else out_of_data = !r->readblock(r->ctx, d->tries > 0);
         if (d->fatal) return 0;                                  /* the reference has exited (src/decoder.c:709-710,748,782): no other parameter set is tried */
         const struct rt_results *a = &d->results[d->parmset];
         if (a->blktype == RT_BS_NONE) { end_of_blocks(d, blklimit); return d->run_all_clean; }      /* what was left of the data was no block */
         ++d->tries;
         ++RT_PARM(d).tried;
         if (attempt_is_final(a)) {
            final = 1;
            if (a->blktype == RT_BS_BLOCK && d->tries > 1) ++d->numblks_goodmultiple;
            break; }
         /* (a PE attempt with a dead track was most likely noise: no second opinion) */
         const int next = d->opt.multiple_tries && (d->opt.mode != RT_PE || a->minbits != 0) ? untried_parmset(d) : -1;
         if (next < 0) break;
         d->parmset = next;
         r->restore_pos(r->ctx);
         d->interblock_counter = 0; }
      if (!final) {
         if (d->tries == 1) { if (d->results[d->parmset].errcount > 0) d->run_all_clean = 0; }
         else {
            int tier;
            const int pick = best_attempt(d, &tier);
            if (tier > 0) d->run_all_clean = 0;
            if (pick < 0) return 0;                                /* ("block state error in process_file()") */
            d->parmset = pick; } }
      if (d->results[d->parmset].blktype == RT_BS_NOISE) continue;
      ++RT_PARM(d).chosen;
      if (d->tries > 1 && decoded_last != d->parmset) {           /* the bit matrix holds another attempt's data */
         r->restore_pos(r->ctx);
         d->interblock_counter = 0;
         rt_init_trackstate(d);
         out_of_data = !r->readblock(r->ctx, 1);
         if (d->fatal) return 0; }
      const enum rt_bstate got = d->results[d->parmset].blktype;
      if (got != RT_BS_TAPEMARK && got != RT_BS_BLOCK && got != RT_BS_BADBLOCK) return 0;
      if (d->on_block) { d->on_block(d, got, d->on_block_user); continue; }      /* (the windowed decode: the finisher puts it out, in tape order) */
      switch (got) {
      case RT_BS_TAPEMARK: rt_got_tapemark(d); break;
      case RT_BS_BLOCK:    rt_got_datablock(d, 0); break;
      default:             rt_got_datablock(d, 1); break; } }
   end_of_blocks(d, blklimit);
   return d->run_all_clean; }

/* ---- the flux-transition statistics' report: <base>.peakstats[_deskew].csv and the head-skew verdict ---- */
#define DESKEW_PEAKDIFF_WARNING 0.20      /* src/decoder.h:44-45: fractions of a bit (double literals, as there) */
#define DESKEW_STDDEV_WARNING   0.05

int rt_output_peakstats(struct rt_dec *d, const char *suffix) {   /* src/decoder.c:175-214 */
   const int B = RT_PEAKSTAT_BUCKETS;
   const float left = d->peakstat.leftbin, bw = d->peakstat.binwidth;
   char filename[1100], cb[32];
   int totalcount = 0;
   snprintf(filename, sizeof filename, "%s.peakstats%s.csv", d->peak_base, suffix);
   FILE *f = fopen(filename, "w");
   if (!f) return 0;
   fprintf(f, "total cnt, <=%.1f uS, >=%.1f uS, track", left * 1e6, bw * 1e6 * (B - 1) + left * 1e6);
   for (int b = 1; b < B - 1; ++b) fprintf(f, ",%.1f uS", bw * 1e6 * b + left * 1e6);
   if (d->opt.mode == RT_NRZI) fprintf(f, ",avg uS");
   fprintf(f, "\n");
   for (int t = 0; t < d->opt.ntrks; ++t) {
      const int *c = d->peakstat.counts[t], sum = d->peakstat.trksums[t];
      long long avgsum = 0;                                     /* (the two catch-all buckets do not count) */
      for (int b = 1; b < B - 1; ++b) avgsum += (long long)(c[b] * (bw * 1e6 * b + left * 1e6));
      fprintf(f, "%d, %d, %d,", sum + c[0] + c[B - 1], c[0], c[B - 1]);
      fprintf(f, "trk%d", t);
      for (int b = 1; b < B - 1; ++b) fprintf(f, ", %.2f%%", sum ? 100 * (float)c[b] / (float)sum : 0);
      if (d->opt.mode == RT_NRZI) fprintf(f, ", %.2f", (float)avgsum / (float)sum);      /* (0 / 0 as the C library prints it) */
      fprintf(f, "\n");
      totalcount += sum; }
   fclose(f);
   if (!d->peak_quiet) {
      rlog(d, "  created statistics file \"%s\" from %s measurements of flux transition positions\n", filename, commas(totalcount, cb));
      rlog(d, "  to graph it from Excel, open the CSV file, then: insert chart 2D line\n"); }
   d->peakstat.initialized = 0;
   return 1; }

int rt_skew_verdict(struct rt_dec *d) {   /* skew_compute_deskew's numbers and its answer (src/decoder.c:243-281) */
   const int B = RT_PEAKSTAT_BUCKETS, ntrks = d->opt.ntrks;
   const float left = d->peakstat.leftbin, bw = d->peakstat.binwidth;
   float avg[RT_MAXTRKS], stddev[RT_MAXTRKS];
   for (int t = 0; t < ntrks; ++t) {
      long long avgsum = 0;
      for (int b = 1; b < B - 1; ++b) avgsum += (long long)(d->peakstat.counts[t][b] * (bw * 1e6 * b + left * 1e6));
      avg[t] = (float)avgsum / (float)d->peakstat.trksums[t]; }
   for (int t = 0; t < ntrks; ++t) {
      stddev[t] = 0;
      for (int b = 1; b < B - 1; ++b) {
         const float deviation = (bw * 1e6f * b + left * 1e6f) - avg[t];
         stddev[t] += d->peakstat.counts[t][b] * (deviation * deviation); }
      stddev[t] = sqrtf(stddev[t] / (float)d->peakstat.trksums[t]); }
   float maxavg = 0, minavg = FLT_MAX, maxstddev = 0;
   for (int t = 0; t < ntrks; ++t) {                            /* (the reference's max / min macros, operands in its order: a NaN average is taken) */
      maxavg = maxavg > avg[t] ? maxavg : avg[t];
      minavg = minavg < avg[t] ? minavg : avg[t];
      maxstddev = maxstddev > stddev[t] ? maxstddev : stddev[t]; }
   const float peak_frac = (maxavg - minavg) / (1e6f / (d->opt.bpi * d->opt.ips));
   const float stddev_frac = maxstddev / (1e6f / (d->opt.bpi * d->opt.ips));
   if (!d->peak_quiet) {
      rlog(d, "  the earliest peak is %.2f usec, and the latest peak is %.2f usec\n", minavg, maxavg);
      rlog(d, "  that peak difference of %.2f usec, and the largest standard deviation of %.2f usec, are %.1f%% and %.1f%% of the nominal bit spacing\n",
           maxavg - minavg, maxstddev, peak_frac * 100, stddev_frac * 100); }
   d->skew_verdict.peak_frac = peak_frac; d->skew_verdict.stddev_frac = stddev_frac;
   d->skew_verdict.ok = peak_frac < DESKEW_PEAKDIFF_WARNING && stddev_frac < DESKEW_STDDEV_WARNING;
   return d->skew_verdict.ok; }

void rt_peakstats_report(struct rt_dec *d) {   /* src/readtape.c:2045-2058; with -q the reference reports nothing here */
   if (d->peak_quiet) { rt_skew_verdict(d); return; }           /* (the caller may still want the numbers) */
   rlog(d, "\n");
   rt_output_peakstats(d, "");
   if (rt_skew_verdict(d)) {
      if (d->peak_deskew) rlog(d, "  deskewing with delays up to %.1f%% of a bit time seems to have been successful\n", d->deskew_max_delay_percent);
      else rlog(d, "  the tape data head skew is minimal\n"); }
   else {
      if (d->peak_deskew) rlog(d, "  deskewing with delays up to %.1f%% of a bit time wasn't entirely effective\n"
                                  "  the tape might have been written by two different drives\n"
                                  "  if so you should consider separating the data into those sections\n", d->deskew_max_delay_percent);
      else rlog(d, "  head skew is significant; you should try again with the -deskew option\n"); } }

/* ---- -deskew pre-pass (src/readtape.c:1675-1717 + skew_compute_deskew / skew_set_delay, src/decoder.c:235-281) ---- */
int rt_deskew_prepass(struct rt_dec *d, struct rt_reader *r, int delays[RT_MAXTRKS], int *hit_end) {
   const int ntrks = d->opt.ntrks;
   int nblks = 0, min_transitions = 0;
   *hit_end = 0;
   d->doing_deskew = 1;
   d->peakstat.initialized = 0;
   d->interblock_counter = 0;
   const int ww = d->opt.mode == RT_WW;
   if (ww) { d->parmset = 0; rt_init_trackstate(d); d->ww_prepassed = 1; }   /* src/readtape.c:1674 */
   do {                                                      /* one block at a time, first parameter set only */
      rt_init_blockstate(d);
      d->parmset = 0;
      if (ww) rt_ww_init_blockstate(d); else rt_init_trackstate(d);
      if (!r->readblock(r->ctx, 1)) { *hit_end = 1; break; }
      if (d->results[d->parmset].blktype != RT_BS_NOISE) {
         min_transitions = INT_MAX;
         for (int t = 0; t < ntrks; ++t) if (d->peakstat.trksums[t] < min_transitions) min_transitions = d->peakstat.trksums[t];
         ++nblks; } }
   while (nblks < RT_MAXSKEWBLKS && min_transitions < RT_MINSKEWTRANS);
   d->doing_deskew = 0;
   d->interblock_counter = 0;
   if (!d->peakstat.initialized) { d->peakstat.initialized = 0; return -1; }
   if (min_transitions <= 0) { d->peakstat.initialized = 0; return -1; }   /* "Some tracks have no transitions" (fatal there) */
   /* the average transition position of each track, over the buckets between the two catch-alls */
   float avg[RT_MAXTRKS], maxavg = 0;
   const float bw = d->peakstat.binwidth, left = d->peakstat.leftbin;
   for (int t = 0; t < ntrks; ++t) {
      long long sum = 0;
      for (int b = 1; b < RT_PEAKSTAT_BUCKETS - 1; ++b)        /* (each term is truncated to an integer number of usec) */
         sum += (long long)(d->peakstat.counts[t][b] * (bw * 1e6 * b + left * 1e6));
      avg[t] = (float)sum / (float)d->peakstat.trksums[t];
      if (avg[t] > maxavg) maxavg = avg[t]; }
   /* delay every track up to the latest one, rounded to whole samples */
   for (int t = 0; t < ntrks; ++t) {
      const float time = d->peakstat.trksums[t] > 0 ? (maxavg - avg[t]) / 1e6f : 0;
      int delay = (int)((time + d->sample_deltat / 2) / d->sample_deltat);
      delays[t] = delay < RT_MAXSKEWSAMP ? delay : RT_MAXSKEWSAMP;
      rlog(d, "  track %d delayed by %d clocks (%.2f usec) based on %d observed flux transitions\n",
           t, delays[t], delays[t] * d->sample_deltat * 1e6, d->peakstat.trksums[t]); }
   if (d->want_peakstats) {                                  /* the rest of skew_compute_deskew(true), then output_peakstats("_deskew") (src/readtape.c:1701-1704) */
      rt_skew_verdict(d);
      d->deskew_max_delay_percent = d->skew_verdict.peak_frac * 100;
      rt_output_peakstats(d, "_deskew"); }
   d->peakstat.initialized = 0;
   if (ww) {                                                 /* the pulse heights learned on the way (src/readtape.c:1706-1716); the caller resets the detector */
      rlog(d, "\n");
      d->ww.t_lastblockmark = 0;
      d->ww.blockmark_queued = 0;
      for (int t = 0; t < ntrks; ++t) {
         struct rt_trk *k = &d->trk[t];
         const int count = k->v_avg_height_count;
         if (count) { k->v_avg_height = k->v_avg_height_sum / count; k->v_avg_height_count = 0; k->v_avg_height_sum = 0; }
         rlog(d, "  trk %d average peak height is %.2fV and AGC is %.2f, based on %d measurements\n", t, k->v_avg_height / 2, k->agc_gain, count); }
      rlog(d, "\n"); }
   return nblks; }

/* ---- density detection (src/readtape.c:1656-1672 + estden_setdensity, src/decoder.c:374-399) ---- */
float rt_density_prepass(struct rt_dec *d, struct rt_reader *r, float *implied, int *nblks, int *hit_end) {
   *nblks = 0; *hit_end = 0; *implied = 0;
   d->doing_density_detection = 1;
   d->opt.bpi = 0;
   memset(&d->estden, 0, sizeof d->estden);
   d->interblock_counter = 0;
   do {
      rt_init_blockstate(d);
      d->parmset = 0;
      rt_init_trackstate(d);
      if (!r->readblock(r->ctx, 1)) { *hit_end = 1; break; }
      if (d->estden.fatal) break;
      if (d->results[d->parmset].blktype != RT_BS_NOISE) ++*nblks; }
   while (d->estden.totalcount < RT_ESTDEN_COUNTNEEDED);
   d->doing_density_detection = 0;
   d->interblock_counter = 0;
   if (d->estden.fatal) return -1;
   /* the smallest transition distance seen at least 5 % of the time (ESTDEN_MINPERCENT) */
   int mindist = INT_MAX;
   for (int i = 0; i < d->estden.binsused; ++i)
      if (d->estden.counts[i] > d->estden.totalcount * 5 / 100 && d->estden.deltas[i] < mindist) mindist = d->estden.deltas[i];
   float density = 1.0f / (d->opt.ips * (float)(mindist + 0.5f) * (float)0.5e-6);
   if (d->opt.mode == RT_PE) density /= 2;                     /* twice the transitions */
   *implied = density;
   static const float standard[] = { 200, 556, 800, 1600, 9042 };
   for (int i = 0; i < 5; ++i) {
      float diff = density - standard[i];
      if (diff < 0) diff = -diff;
      if (diff < standard[i] * 20 / 100) {                     /* ESTDEN_CLOSEPERCENT */
         d->opt.bpi = standard[i];
         char cb[32];
         rlog(d, "  density was set to %.0f BPI (%.2f usec/bit) after reading the first %d blocks and seeing %s transitions in %d bins that imply %.0f BPI\n",
              d->opt.bpi, 1e6 / (d->opt.bpi * d->opt.ips), *nblks, commas(d->estden.totalcount, cb), d->estden.binsused, density);
         return d->opt.bpi; } }
   return 0; }
