/* rt_csv.c — CSV ingest: a logic-analyser export ("time, v0, v1, ..." behind two title lines) becomes the
 * int16 rows + TBIN header fields the device front end takes.  The numbers are the ones the reference's converter writes
 * (src/csvtbin.c:619-716): the sample period from the first and last timestamps of the pre-read, the full-scale voltage from
 * the largest magnitude seen (plus 0.5 V, rounded to 0.1 V) unless a larger one is given, and round-half-away quantisation
 * clamped to +-32767.  Text -> number conversion accumulates digit by digit in the precision of the result, as the reference's
 * scanner does (src/csvtbin.c scanfast_*): a correctly rounded strtof() would differ in the last bit now and then.
 */
#include "rt_csv.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

enum { LINE_MAX_CHARS = 400,            /* MAXLINE,       src/csvtbin.c:123 */
       PREREAD_ROWS   = 1000000 };      /* PREREAD_COUNT, src/csvtbin.c:125 */

/* one decimal number at *p (blanks and commas in front of it skipped), accumulated in `double` */
static double scan_f64(const char **p) {
   const char *s = *p;
   while (*s == ' ' || *s == ',') ++s;
   const int neg = *s == '-';
   if (neg) ++s;
   double v = 0;
   for (; *s >= '0' && *s <= '9'; ++s) v = v * 10 + (*s - '0');
   if (*s == '.') {
      double scale = 10;
      for (++s; *s >= '0' && *s <= '9'; ++s, scale *= 10) v += (*s - '0') / scale; }
   *p = s;
   return neg ? -v : v; }

/* ... accumulated in `float` */
static float scan_f32(const char **p) {
   const char *s = *p;
   while (*s == ' ' || *s == ',') ++s;
   const int neg = *s == '-';
   if (neg) ++s;
   float v = 0;
   for (; *s >= '0' && *s <= '9'; ++s) v = v * 10 + (*s - '0');
   if (*s == '.') {
      float scale = 10;
      for (++s; *s >= '0' && *s <= '9'; ++s, scale *= 10) v += (*s - '0') / scale; }
   *p = s;
   return neg ? -v : v; }

static int next_line(FILE *f, char *line) {
   if (!fgets(line, LINE_MAX_CHARS, f)) return 0;
   line[LINE_MAX_CHARS - 1] = 0;
   return 1; }

double rt_csv_scan_time(const char *line) { return scan_f64(&line); }

int rt_csv_survey(const char *path, int ntrks, float scale, int subsample, float maxvolts_given, struct rt_csv_info *out) {
   return rt_csv_survey_n(path, ntrks, scale, subsample, maxvolts_given, PREREAD_ROWS, out); }

int rt_csv_survey_n(const char *path, int ntrks, float scale, int subsample, float maxvolts_given, int64_t preread_rows, struct rt_csv_info *out) {
   char line[LINE_MAX_CHARS + 1];
   FILE *f = fopen(path, "r");
   if (!f) return -1;
   memset(out, 0, sizeof *out);
   if (!next_line(f, line) || !next_line(f, line)) { fclose(f); return -2; }        /* the two title lines */
   for (const char *c = line; *c; ++c) out->columns += *c == ',';
   double t_first = -1;
   float peak = 0;
   int64_t n = 0;
   uint32_t tdelta = 0;
   while (next_line(f, line) && ++n < preread_rows) {
      const char *p = line;
      const double t = scan_f64(&p);
      if (t_first < 0) { t_first = t; out->tstart_ns = (uint64_t)((t_first + 0.5e-9) * 1e9); }
      else tdelta = (uint32_t)(((t - t_first) / (double)(n - 1) + 0.5e-9) * 1e9);
      for (int k = 0; k < ntrks; ++k) {
         float v = scan_f32(&p) * scale;
         if (v < 0) v = -v;
         if (peak < v) peak = v; } }
   /* the rows of the whole file (the pre-read stops at a million) */
   int64_t rows = n;                                   /* (n counted the line on which the pre-read stopped, too) */
   if (n >= preread_rows) while (next_line(f, line)) ++rows;
   fclose(f);
   peak = ((float)(int)((peak + 0.55f) * 10.0f)) / 10.0f;
   if (subsample > 1) { out->tstart_ns += (uint64_t)(subsample - 1) * tdelta; tdelta *= (uint32_t)subsample; }
   out->tdelta_ns = tdelta;
   out->maxvolts = maxvolts_given > peak ? maxvolts_given : peak;
   out->rows = rows / (subsample > 1 ? subsample : 1);
   return 0; }

/* One data line -> its ntrks codes, the one scan-and-quantise loop of the converter (src/csvtbin.c:691-712): column k of the file goes to column perm[k],
 * round half away from zero, clamp to +-32767 (a code that meets a rail counts, +-32767 included).  st follows the codes at either rail, the
 * smallest and the largest sample in volts and the largest magnitude (the caller starts them, and starts amax again per graph bin). */
struct line_stats { int64_t too_big, too_small; float lo, hi, amax; };
static void line_codes(const char *line, int ntrks, const int *perm, int invert, float scale, float maxvolts, int16_t *codes, struct line_stats *st) {
   float v[RT_CSV_MAXTRKS];
   const char *p = line;
   (void)scan_f64(&p);                                                         /* the timestamp: the period is fixed by now */
   for (int k = 0; k < ntrks; ++k) v[perm ? perm[k] : k] = scan_f32(&p) * scale;
   for (int k = 0; k < ntrks; ++k) {
      const float x = invert ? -v[k] : v[k];
      int q = (int)((x / maxvolts * 32767) + (x < 0 ? -0.5f : 0.5f));           /* (all float: (int) truncates towards zero) */
      if (x < st->lo) st->lo = x;
      if (x > st->hi) st->hi = x;
      const float a = x < 0 ? -x : x;
      if (a > st->amax) st->amax = a;
      if (q <= -32767) { q = -32767; ++st->too_small; }
      if (q >= 32767) { q = 32767; ++st->too_big; }
      codes[k] = (int16_t)q; } }

int64_t rt_csv_load(const char *path, int ntrks, const int *perm, int invert, float scale, int subsample, float maxvolts,
                    int16_t *rows, int64_t capacity, int64_t *clipped) {
   char line[LINE_MAX_CHARS + 1];
   if (ntrks < 1 || ntrks > RT_CSV_MAXTRKS) return -3;                          /* (a line's codes: RT_CSV_MAXTRKS columns) */
   if (perm) for (int k = 0; k < ntrks; ++k) if (perm[k] < 0 || perm[k] >= ntrks) return -4;
   FILE *f = fopen(path, "r");
   if (!f) return -1;
   if (!next_line(f, line) || !next_line(f, line)) { fclose(f); return -2; }
   if (subsample < 1) subsample = 1;
   int64_t n = 0;
   struct line_stats st = { 0, 0, 0, 0, 0 };
   for (;;) {
      int got = 1;
      for (int s = 0; s < subsample && got; ++s) got = next_line(f, line);      /* of every `subsample` lines the last one counts */
      if (!got || n >= capacity) break;
      line_codes(line, ntrks, perm, invert, scale, maxvolts, rows + n * ntrks, &st);
      ++n; }
   fclose(f);
   if (clipped) *clipped = st.too_big + st.too_small;
   return n; }

/* ---- the converter's window options, -graph and -redo (src/csvtbin.c:364-376, 661-747) ---- */

/* seconds as the option parser turns them into nanoseconds (src/csvtbin.c:371,374): the float the user gave, widened, times 1e9, cut */
uint64_t rt_csv_seconds_ns(float x) { return (uint64_t)((double)x * 1e9); }

/* full scale for the second pass of -redo (src/csvtbin.c:737): 0.1 V above the largest magnitude seen, cut to 0.1 V; sum and product in double */
float rt_csv_redo_maxvolts(float newmax) { return ((float)(int)((newmax + 0.15) * 10.0f)) / 10.0f; }

/* Which raw data lines a conversion with -skip / -starttime / -endtime / -stopaft keeps, in closed form.  The reference's two loops (:671-680,
 * :685-723) restated:
 *   - with -skip or -starttime the skipping loop is a do-while over RAW lines that adds the (already multiplied) period per line: it drops
 *     K = max(1, skip, ceil((starttime - T0) / D)) lines; the file ending inside it is fatal (-5 here);
 *   - behind them, of every `sub` lines the last one is a sample (a group the file's end cuts is dropped): sample j is raw line K + j sub + sub - 1;
 *   - a sample is written, THEN the clock T0 + (K + m) D is looked at: the pass ends behind the first sample m >= 1 with m >= stopaft (looked at
 *     first) or a clock strictly behind endtime.
 * skip <= 0, starttime <= 0, endtime <= 0, stopaft <= 0: not given. */
int rt_csv_convert_window(uint64_t tstart_ns, uint32_t tdelta_ns, int64_t data_lines, int subsample, int64_t skip, float starttime, float endtime,
                          int64_t stopaft, struct rt_csv_window *out) {
   if (!out || data_lines < 0) return -1;
   typedef unsigned __int128 u128;
   const int64_t sub = subsample > 1 ? subsample : 1;
   const uint64_t start_ns = starttime > 0 ? rt_csv_seconds_ns(starttime) : 0;
   const uint64_t end_ns = endtime > 0 ? rt_csv_seconds_ns(endtime) : UINT64_MAX;
   const uint64_t D = tdelta_ns;
   int64_t K = 0;
   if (skip > 0 || start_ns > 0) {
      K = skip > 1 ? skip : 1;
      if (start_ns > tstart_ns) {                                   /* the first k with T0 + k D >= start_ns */
         if (!D) return -5;                                         /* (the clock stands still: the loop runs into the end of the file) */
         const uint64_t k = (start_ns - tstart_ns + D - 1) / D;
         if (k > (uint64_t)data_lines) return -5;
         if ((int64_t)k > K) K = (int64_t)k; } }
   if (K > data_lines) return -5;
   memset(out, 0, sizeof *out);
   out->skipped = K;
   out->first_line = K + sub - 1;
   const int64_t avail = (data_lines - K) / sub;
   if (avail == 0) return 0;
   /* the first m >= 1 that a stop ends the pass behind */
   uint64_t m_stop = stopaft > 0 ? (uint64_t)stopaft : UINT64_MAX, m_end = UINT64_MAX;
   const u128 t_k = (u128)tstart_ns + (u128)(uint64_t)K * D;        /* the clock behind the skip (beyond 2^64 the reference's wraps: 580 years of tape) */
   if (t_k + D > end_ns) m_end = 1;
   else if (D) m_end = (uint64_t)((end_ns - t_k) / D) + 1;          /* (end_ns = UINT64_MAX: not given, and no clock of 64 bits gets behind it) */
   if (end_ns == UINT64_MAX) m_end = UINT64_MAX;
   const uint64_t m_break = m_stop < m_end ? m_stop : m_end;
   if (m_break <= (uint64_t)avail) { out->count = (int64_t)m_break; out->ended = m_stop <= m_end ? RT_CSV_ENDED_STOPAFT : RT_CSV_ENDED_ENDTIME; }
   else { out->count = avail; out->ended = RT_CSV_ENDED_FILE; }
   return 0; }

/* One pass of the conversion, the way the reference runs it: a stream of lines, nothing known in advance.  Whatever of the sinks is given is filled:
 * rows[capacity][ntrks]; tbin_path (created: `header`, the rows, the end mark 0x8000); graph_path (created; a line "<sample number>, <%f of the bin's
 * maximum>" per full bin of o->graphbin samples) and graph_at[] / graph_max[] (the same lines as numbers, at most graph_cap of them).
 * Returns 0, or -1 (cannot open the CSV) -2 (no title lines) -3 (ntrks) -4 (perm) -5 (the file ends inside the skip) -6 (cannot create an output file)
 * -7 (a write failed) -8 (more samples than `capacity`). */
int rt_csv_convert_pass(const char *csv_path, const struct rt_csv_pass_opts *o, int16_t *rows, int64_t capacity, const char *tbin_path, const void *header,
                        int header_bytes, const char *graph_path, int64_t *graph_at, float *graph_max, int64_t graph_cap, struct rt_csv_pass *res) {
   char line[LINE_MAX_CHARS + 1];
   if (!o || !res) return -1;
   const int ntrks = o->ntrks;
   if (ntrks < 1 || ntrks > RT_CSV_MAXTRKS) return -3;
   if (o->perm) for (int k = 0; k < ntrks; ++k) if (o->perm[k] < 0 || o->perm[k] >= ntrks) return -4;
   memset(res, 0, sizeof *res);
   FILE *f = fopen(csv_path, "r"), *tf = NULL, *gf = NULL;
   if (!f) return -1;
   int rc = 0;
   char *buf = NULL;
   if (!next_line(f, line) || !next_line(f, line)) { rc = -2; goto out; }
   if (tbin_path) {
      if (!(tf = fopen(tbin_path, "wb"))) { rc = -6; goto out; }
      if ((buf = (char *)malloc(1 << 20))) setvbuf(tf, buf, _IOFBF, 1 << 20);
      if (header_bytes > 0 && fwrite(header, (size_t)header_bytes, 1, tf) != 1) { rc = -7; goto out; } }
   if (graph_path && o->graphbin > 0 && !(gf = fopen(graph_path, "w"))) { rc = -6; goto out; }
   const uint64_t start_ns = o->starttime > 0 ? rt_csv_seconds_ns(o->starttime) : 0;
   const uint64_t end_ns = o->endtime > 0 ? rt_csv_seconds_ns(o->endtime) : UINT64_MAX;
   const uint64_t stopaft = o->stopaft > 0 ? (uint64_t)o->stopaft : UINT64_MAX;
   const int sub = o->subsample > 1 ? o->subsample : 1;
   uint64_t clock = o->tstart_ns;
   if (o->skip > 0 || start_ns > 0) {
      int64_t left = o->skip > 0 ? o->skip : 0;
      do {
         if (!fgets(line, LINE_MAX_CHARS, f)) { rc = -5; goto out; }
         clock += o->tdelta_ns;
         ++res->skipped;
         if (left > 0) --left; }
      while (clock < start_ns || left > 0); }
   struct line_stats st = { 0, 0, 0, 0, 0 };                                   /* (amax: the graph's bin, started again behind each printed line) */
   int64_t in_bin = 0;
   uint64_t n = 0;
   for (;;) {
      int got = 1;
      for (int s = 0; s < sub && got; ++s) got = next_line(f, line);
      if (!got) break;
      int16_t codes[RT_CSV_MAXTRKS];
      line_codes(line, ntrks, o->perm, o->invert, o->scale, o->maxvolts, codes, &st);
      if (rows) {
         if ((int64_t)n >= capacity) { rc = -8; goto out; }
         memcpy(rows + n * ntrks, codes, sizeof(int16_t) * (size_t)ntrks); }
      if (tf && fwrite(codes, sizeof(int16_t), (size_t)ntrks, tf) != (size_t)ntrks) { rc = -7; goto out; }      /* (little-endian hosts) */
      clock += o->tdelta_ns;
      ++n;
      if (n >= stopaft) { res->ended = RT_CSV_ENDED_STOPAFT; break; }
      if (clock > end_ns) { res->ended = RT_CSV_ENDED_ENDTIME; break; }
      if (o->graphbin > 0 && ++in_bin >= o->graphbin) {               /* behind the two stops: the sample that ends the pass prints no line */
         if (gf && fprintf(gf, "%llu, %f\n", (unsigned long long)n, st.amax) < 0) { rc = -7; goto out; }
         if (res->graph_lines < graph_cap) {
            if (graph_at) graph_at[res->graph_lines] = (int64_t)n;
            if (graph_max) graph_max[res->graph_lines] = st.amax; }
         ++res->graph_lines;
         st.amax = 0;
         in_bin = 0; } }
   res->samples = (int64_t)n;
   res->too_big = st.too_big; res->too_small = st.too_small;
   res->newmax = st.hi > -st.lo ? st.hi : -st.lo;
   if (tf) { const int16_t end = (int16_t)0x8000; if (fwrite(&end, 2, 1, tf) != 1) rc = -7; }
out:
   fclose(f);
   if (tf) { const int bad = ferror(tf); if ((fclose(tf) || bad) && !rc) rc = -7; }
   if (gf) { const int bad = ferror(gf); if ((fclose(gf) || bad) && !rc) rc = -7; }
   free(buf);
   return rc; }

/* the graph file from the bins' maxima (the device path's: bin i closes on sample (i + 1) * graphbin) */
int rt_csv_graph_write(const char *graph_path, int64_t graphbin, const float *bins, int64_t nbins) {
   FILE *gf = fopen(graph_path, "w");
   if (!gf) return -6;
   int bad = 0;
   for (int64_t i = 0; i < nbins && !bad; ++i) bad = fprintf(gf, "%llu, %f\n", (unsigned long long)((i + 1) * graphbin), bins[i]) < 0;
   if (ferror(gf)) bad = 1;
   return (fclose(gf) || bad) ? -7 : 0; }
