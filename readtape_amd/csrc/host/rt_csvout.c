/* rt_csvout.c — int16 rows -> the text of the converter's -read (src/csvtbin.c:523-596), on the host.
 *
 * The plain path: one fprintf per field, as the reference does it.  It is what csvout.write_csv runs, and what the device path
 * (rtfe_csv_format, csrc/rtfe_csvout.hip) is compared with where the reference itself is not at hand.  The text:
 *   '<descr>
 *   Time, Track 0, ..., Track n-1
 *   <%12.8f of (double)t_ns / 1e9>, <%9.5f of column 0>, ..., <%9.5f of column n-1>, \n      (the last field keeps its ", ")
 * a column's value being, in float32 with two roundings, code / 32767 * maxvolts, negated for an inverted tape, plus k times the stagger
 * (the stagger itself summed in float32, column after column). */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "rt_csv.h"

/* seconds as the option parser turns them into nanoseconds (src/csvtbin.c:371,374): the float the user gave, widened, times 1e9, cut */
static uint64_t seconds_to_ns(float x) { return (uint64_t)((double)x * 1e9); }

/* Which rows a -read with -skip / -starttime / -endtime / -stopaft prints, of a tape of nrows rows (the end mark already taken off).
 * skip <= 0, starttime <= 0, endtime <= 0, stopaft <= 0: not given.  Returns 0 and rows [*first, *first + *count).
 *   - the skipping loop is a do-while (src/csvtbin.c:559-567): with either -skip or -starttime at least one row goes, then rows go until
 *     the time has reached starttime AND skip rows have gone;
 *   - a row is printed, THEN the clock advances and the two stops are looked at (:593-594): the row that crosses endtime is still printed. */
int rt_csv_export_window(uint64_t tstart_ns, uint32_t tdelta_ns, int64_t nrows, int64_t skip, float starttime, float endtime, int64_t stopaft,
                         int64_t *first, int64_t *count) {
   if (!first || !count || nrows < 0) return -1;
   const uint64_t start_ns = starttime > 0 ? seconds_to_ns(starttime) : 0;
   const uint64_t end_ns = endtime > 0 ? seconds_to_ns(endtime) : UINT64_MAX;
   int64_t i = 0;
   if (skip > 0 || start_ns > 0) {
      i = skip > 1 ? skip : 1;
      if (start_ns > tstart_ns) {                                   /* the first i with tstart + i * tdelta >= start_ns */
         const uint64_t d = start_ns - tstart_ns;
         const uint64_t k = tdelta_ns ? (d + tdelta_ns - 1) / tdelta_ns : (uint64_t)INT64_MAX;
         if (k > (uint64_t)i) i = k > (uint64_t)INT64_MAX ? INT64_MAX : (int64_t)k; } }
   if (i >= nrows) { *first = nrows; *count = 0; return 0; }
   int64_t n = nrows - i;
   if (stopaft > 0 && stopaft < n) n = stopaft;
   const uint64_t t_i = tstart_ns + (uint64_t)i * tdelta_ns;
   if (t_i > end_ns) n = 1;                                          /* (n >= 1 here) */
   else if (tdelta_ns) {                                            /* the first n >= 1 with t_i + n * tdelta > end_ns */
      const uint64_t m = (end_ns - t_i) / tdelta_ns + 1;
      if (m < (uint64_t)n) n = (int64_t)m; }
   *first = i; *count = n;
   return 0; }

/* The file: two title lines and rows [first, first + count) of rows[.][ntrks]; column k prints rows[.][perm ? perm[k] : k].
 * Returns the bytes written, or -1 (cannot create), -2 (a write failed), -3 (ntrks), -4 (perm). */
int64_t rt_csv_export_write(const char *path, const char *descr, int ntrks, const int *perm, int invert, float maxvolts, float stagger,
                            uint64_t tstart_ns, uint32_t tdelta_ns, const int16_t *rows, int64_t first, int64_t count) {
   if (ntrks < 1 || ntrks > RT_CSV_MAXTRKS) return -3;
   if (perm) for (int k = 0; k < ntrks; ++k) if (perm[k] < 0 || perm[k] >= ntrks) return -4;
   FILE *f = fopen(path, "wb");
   if (!f) return -1;
   char *buf = (char *)malloc(1 << 20);                             /* (stdio's own 4 KB buffer is a write() per 36 rows) */
   if (buf) setvbuf(f, buf, _IOFBF, 1 << 20);
   int64_t bytes = 0;
   int n = fprintf(f, "'%s\nTime, ", descr ? descr : "");
   bytes += n;
   for (int k = 0; k < ntrks && n >= 0; ++k) { n = fprintf(f, "Track %d%s", k, k == ntrks - 1 ? "" : ", "); bytes += n; }
   if (n >= 0) { n = fprintf(f, "\n"); bytes += n; }
   for (int64_t r = first; r < first + count && n >= 0; ++r) {
      const int16_t *row = rows + r * ntrks;
      const uint64_t t = tstart_ns + (uint64_t)r * tdelta_ns;
      n = fprintf(f, "%12.8f, ", (double)t / 1e9);
      bytes += n;
      float amount = 0.f;
      for (int k = 0; k < ntrks && n >= 0; ++k) {
         float v = (float)row[perm ? perm[k] : k] / 32767 * maxvolts;
         if (invert) v = -v;
         v += amount;
         amount += stagger;
         n = fprintf(f, "%9.5f, ", v);
         bytes += n; }
      if (n >= 0) { n = fprintf(f, "\n"); bytes += n; } }
   const int bad = n < 0 || ferror(f);
   const int closed = fclose(f);
   free(buf);
   if (closed != 0 || bad) return -2;
   return bytes; }
