/* rt_textfile.c — the interpreted text dump (src/textfile.c), restated around a context and by lines: a record is cut into
 * its lines first (where the reference's byte loop would break them), and every line is then made in one piece - the numbers,
 * the blanks that line the character column up, the characters - and written at once.  The device formatter
 * (../rtfe_textfile.hip) makes the same lines, a lane a line; tests/make_textfile_golden.py pins both to the reference's bytes.
 *
 * Where the reference's loop breaks a line (src/textfile.c:252-259): in front of the byte at which the line already holds
 * linesize bytes, or, with -linefeed, in front of a 0x0a.  Under -octal2 the loop steps two bytes at a time and tests only the
 * first of a pair: a 0x0a at an odd index breaks nothing, and a line of an odd linesize runs one byte over (the blanks counted
 * for the bytes "missing" from it then come out negative: none are written).  A 0x0a that is a record's first byte leaves the
 * prefix alone on its line. */
#include "rt_textfile.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

struct rt_textfile {
   rt_text_options o;
   int doboth, tapread;
   unsigned char table[512];
   char name[1200], created[64];
   FILE *f;
   int failed;
   int numrecords, numerrors, numwarnings, numboth, numtapemarks, numchars;
   long long numbytes, written;
   char line[64 + 6 * RT_TEXT_MAXLINE];      /* prefix, 3 digits and a blank a byte (or as many blanks), 2 blanks, a character a byte, the line end */
};

int rt_text_name(const char *base, const rt_text_options *in, char *out, size_t outlen) {
   rt_text_options o;
   if (rt_text_resolve(in, &o)) return -1;
   const int both = o.numtype != RT_NUM_NONE && o.chartype != RT_CHAR_NONE, any = o.numtype != RT_NUM_NONE || o.chartype != RT_CHAR_NONE;
   const int n = snprintf(out, outlen, "%s.%s%s%s%stxt", base, rt_text_num_names[o.numtype] + 1, both ? "." : "", rt_text_char_names[o.chartype] + 1, any ? "." : "");
   return n < 0 || (size_t)n >= outlen ? -1 : 0; }

struct rt_textfile *rt_text_new(const char *base, const rt_text_options *in, int tapread, const char *created) {
   struct rt_textfile *t = (struct rt_textfile *)calloc(1, sizeof *t);
   if (!t) return NULL;
   if (rt_text_resolve(in, &t->o) || rt_text_name(base, &t->o, t->name, sizeof t->name)) { free(t); return NULL; }
   t->doboth = t->o.numtype != RT_NUM_NONE && t->o.chartype != RT_CHAR_NONE;
   t->tapread = tapread != 0;
   rt_text_char_table(t->o.chartype, t->table);
   if (created) snprintf(t->created, sizeof t->created, "%s", created);
   else { time_t now = time(NULL); char buf[32]; snprintf(t->created, sizeof t->created, "%s", ctime_r(&now, buf)); }
   return t; }

const char *rt_text_filename(const struct rt_textfile *t) { return t->name; }

static void put(struct rt_textfile *t, const void *p, size_t n) {
   if (!t->f || t->failed || !n) return;
   if (fwrite(p, 1, n, t->f) != n) t->failed = 1;
   t->written += (long long)n; }
static void puts_(struct rt_textfile *t, const char *s) { put(t, s, strlen(s)); }

int rt_text_open_now(struct rt_textfile *t) {            /* the three title lines, src/textfile.c:199-209 */
   if (t->f) return 0;
   if (t->failed) return -1;
   t->f = fopen(t->name, "w");
   if (!t->f) { t->failed = 1; return -1; }
   char buf[1400];
   snprintf(buf, sizeof buf, "file %s\n", t->name); puts_(t, buf);
   snprintf(buf, sizeof buf, "created by readtape%s version %s on %s", t->tapread ? " -tapread" : "", RT_TEXT_VERSION, t->created); puts_(t, buf);
   snprintf(buf, sizeof buf, "using text options %s %s%s -linesize=%d", rt_text_num_names[t->o.numtype], rt_text_char_names[t->o.chartype],
            t->o.linefeed ? " -newline" : "", t->o.linesize); puts_(t, buf);
   if (t->o.dataspace) { snprintf(buf, sizeof buf, " -dataspace=%d", t->o.dataspace); puts_(t, buf); }
   if (t->o.numtype == RT_NUM_NONE && t->o.chartype == RT_CHAR_NONE) puts_(t, "\nno numeric or character options were given, so we will display only block sizes");
   puts_(t, "\n\n");
   return t->failed ? -1 : 0; }

static void end_size_list(struct rt_textfile *t) {       /* the sizes-only list's unfinished line */
   if (t->numchars > 0) { puts_(t, "\n"); t->numchars = 0; } }

void rt_text_message(struct rt_textfile *t, const char *msg) {
   if (rt_text_open_now(t)) return;
   end_size_list(t);
   puts_(t, msg); }

void rt_text_tapemark(struct rt_textfile *t, double timenow) {
   ++t->numtapemarks;
   if (t->tapread) rt_text_message(t, RT_TAP_MARK_TEXT);
   else { char buf[80]; snprintf(buf, sizeof buf, "tape mark at time %.8lf\n", timenow); rt_text_message(t, buf); } }

void rt_text_count(struct rt_textfile *t, int length, int errs, int warnings) {
   ++t->numrecords;
   t->numbytes += length;
   if (errs > 0 && warnings > 0) ++t->numboth;
   else { if (errs > 0) ++t->numerrors; if (warnings > 0) ++t->numwarnings; } }

void rt_text_count_items(struct rt_textfile *t, const rt_tap_item *items, int64_t n) {
   for (int64_t i = 0; i < n; ++i) {
      if (items[i].kind == RT_TAP_RECORD) rt_text_count(t, (int)items[i].length, items[i].flag ? 1 : 0, 0);
      else if (items[i].kind == RT_TAP_MARK) ++t->numtapemarks; } }

void rt_text_body(struct rt_textfile *t, const void *text, size_t n) {
   if (rt_text_open_now(t)) return;
   put(t, text, n); }

/* how many bytes the line that starts at index start of a record of length bytes holds; first: the record's first line, whose
 * first byte is tested like every other (a line made by a break holds the byte that broke it) */
static int line_extent(const struct rt_textfile *t, const unsigned char *bytes, int length, int start, int first) {
   const int step = t->o.numtype == RT_NUM_OCTAL2 ? 2 : 1;
   int n = 0;
   for (int i = start; i < length; i += step) {
      if ((i > start || first) && (n >= t->o.linesize || (t->o.linefeed && bytes[i] == 0x0a))) break;
      n += i + step <= length ? step : 1; }
   return n; }

/* the line of bytes[start .. start + n) behind its prefix: numbers, the blanks up to the character column, characters */
static size_t make_line(struct rt_textfile *t, const unsigned char *bytes, int length, int start, int n, char *o) {
   static const char hexd[] = "0123456789ABCDEF";
   const rt_text_options *q = &t->o;
   const int narrow = q->ntrks <= 7;
   char *p = o;
   if (q->numtype == RT_NUM_NONE)
      for (int j = 0; j < n; ++j) *p++ = (char)t->table[((start + j) & 1) * 256 + bytes[start + j]];
   else {
      for (int j = 0; j < n;) {
         const unsigned b = bytes[start + j];
         if (q->numtype == RT_NUM_HEX) { *p++ = hexd[b >> 4]; *p++ = hexd[b & 15]; ++j; }
         else if (q->numtype == RT_NUM_OCTAL || start + j == length - 1) {      /* a byte alone: octal, or octal2's odd last byte */
            if (!narrow) *p++ = (char)('0' + (b >> 6));
            else if (b >> 6) *p++ = (char)('0' + (b >> 6));                      /* ("%02o" of a value above 077 takes its third digit) */
            *p++ = (char)('0' + ((b >> 3) & 7)); *p++ = (char)('0' + (b & 7)); ++j; }
         else {                                                                  /* octal2: a 16-bit word, six digits */
            const unsigned w = b << 8 | bytes[start + j + 1];
            for (int s = 15; s >= 0; s -= 3) *p++ = (char)('0' + ((w >> s) & 7));
            j += 2; }
         if (q->dataspace > 0 && j % q->dataspace == 0) *p++ = ' '; }
      if (t->doboth) {
         const int missing = q->linesize - n;
         int blanks = (q->dataspace ? missing / q->dataspace : 0) + missing * (q->numtype == RT_NUM_HEX || narrow ? 2 : 3);
         for (; blanks > 0; --blanks) *p++ = ' ';
         if (q->dataspace == 0) { *p++ = ' '; *p++ = ' '; }
         for (int j = 0; j < n; ++j) *p++ = (char)t->table[((start + j) & 1) * 256 + bytes[start + j]]; } }
   *p++ = '\n';
   return (size_t)(p - o); }

void rt_text_record(struct rt_textfile *t, const unsigned char *bytes, int length, int errs, int warnings, const char *head) {
   if (rt_text_open_now(t)) return;
   rt_text_count(t, length, errs, warnings);
   const char flag = errs > 0 && warnings > 0 ? 'X' : errs > 0 ? '!' : warnings > 0 ? '?' : ' ';
   if (t->o.numtype == RT_NUM_NONE && t->o.chartype == RT_CHAR_NONE) {      /* sizes only: a list broken where a line has reached linesize characters */
      char buf[40];
      if (t->numchars > 0) { puts_(t, ", "); t->numchars += 2; }
      t->numchars += snprintf(buf, sizeof buf, "%c%d", flag, length);
      puts_(t, buf);
      if (t->numchars >= t->o.linesize) { puts_(t, "\n"); t->numchars = 0; }
      return; }
   const char *cont = head ? " " : "       ";
   if (head) { puts_(t, head); puts_(t, "\n"); }
   for (int start = 0, first = 1;; first = 0) {
      char *o = t->line;
      if (first && !head) o += sprintf(o, "%c%4d: ", flag, length);
      else { const size_t k = strlen(cont); memcpy(o, cont, k); o += k; }
      const int n = line_extent(t, bytes, length, start, first);
      o += make_line(t, bytes, length, start, n, o);
      put(t, t->line, (size_t)(o - t->line));
      start += n;
      if (start >= length) break; } }

static const char *commas(long long n, char buf[32]) {
   char raw[24];
   const int len = snprintf(raw, sizeof raw, "%lld", n);
   int o = 0;
   for (int i = 0; i < len; ++i) { buf[o++] = raw[i]; if ((len - 1 - i) % 3 == 0 && i != len - 1) buf[o++] = ','; }
   buf[o] = 0;
   return buf; }

long long rt_text_close(struct rt_textfile *t, int trailer) {      /* src/textfile.c:277-305 */
   if (!t) return 0;
   if (t->f && trailer) {
      char buf[200], cb[32];
      end_size_list(t);
      puts_(t, "end of file\n\n");
      snprintf(buf, sizeof buf, "there were %d data blocks with %s bytes, and %d tapemarks\n", t->numrecords, commas(t->numbytes, cb), t->numtapemarks); puts_(t, buf);
      const int b = t->numboth, e = t->numerrors, w = t->numwarnings;
      if (!t->tapread) {
         if (b > 0) { snprintf(buf, sizeof buf, "%d block%s had both errors and warnings\n", b, b == 1 ? "" : "s"); puts_(t, buf); }
         if (e > 0) { snprintf(buf, sizeof buf, "%d block%s had errors\n", e, e == 1 ? "" : "s"); puts_(t, buf); }
         else if (b == 0) puts_(t, "no blocks had errors\n");
         if (w > 0) { snprintf(buf, sizeof buf, "%d block%s had warnings\n", w, w == 1 ? "" : "s"); puts_(t, buf); }
         else if (b == 0) puts_(t, "no blocks had warnings\n"); }
      else {
         if (b > 0) { snprintf(buf, sizeof buf, b == 1 ? "%d block with both errors and warnings was marked with a X before the length\n"
                                                        : "%d blocks with both errors and warnings were marked with a X before the length\n", b); puts_(t, buf); }
         if (e > 0) { snprintf(buf, sizeof buf, e == 1 ? "%d block with errors was marked with a ! before the length\n"
                                                        : "%d blocks with errors were marked with a ! before the length\n", e); puts_(t, buf); }
         else if (b == 0) puts_(t, "no blocks had errors\n");
         if (w > 0) { snprintf(buf, sizeof buf, w == 1 ? "%d block with warnings was marked with a ? before the length\n"
                                                        : "%d blocks with warnings were marked with a ? before the length\n", w); puts_(t, buf); }
         else if (b == 0) puts_(t, "no blocks had warnings\n"); } }
   long long n = t->written;
   if (t->f && fclose(t->f) != 0) t->failed = 1;
   if (t->failed) n = -1;
   free(t);
   return n; }
