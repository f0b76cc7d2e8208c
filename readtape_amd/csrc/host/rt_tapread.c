/* rt_tapread.c — a SIMH .tap image taken apart (src/tapread.c), and -tapread: its interpreted text file.
 *
 * The image is walked once into a table of items - records, tape marks and the messages the reference writes into the text -
 * and the table is what gets formatted, here (rt_tapread_write) or on the device (readtape_amd/textfile.py).  Markers are
 * little-endian; bit 31 of a record's marker is its error flag, bits 24..30 must be clear, bits 0..23 are the length.  Behind a
 * record's data the same length must follow, after no or a few pad bytes: the reference shifts a byte in up to four times.  An
 * image that ends without the end-of-medium marker is said to; one that ends anywhere else is a fatal error, as are the
 * erased-gap marker 0xfffffffe (announced in the text, then refused as a bad marker), a zero length and one of 128 KB or more. */
#include "rt_textfile.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static uint32_t le32(const unsigned char *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

struct walk { rt_tap_item *out; int64_t cap, n; };
static void emit(struct walk *w, uint16_t kind, uint64_t offset, uint32_t length, uint16_t flag) {
   if (w->n < w->cap) { rt_tap_item it = { offset, length, kind, flag }; w->out[w->n] = it; }
   ++w->n; }

int64_t rt_tap_items(const unsigned char *img, uint64_t nbytes, rt_tap_item *out, int64_t cap, int *status, char *err, size_t errlen) {
   struct walk w = { out, out ? cap : 0, 0 };
   uint64_t pos = 0;
   long long databytes = 0;                                   /* bytes read one at a time: what the last fatal message calls the file offset */
   int st = RT_TAP_OK;
   char msg[120] = "";
   for (;;) {
      if (nbytes - pos < 4) { emit(&w, RT_TAP_MESSAGE, nbytes, 0, RT_TAP_MSG_NO_END); break; }
      const uint32_t marker = le32(img + pos);
      if (marker == 0xffffffffu) break;
      if (marker == 0) { emit(&w, RT_TAP_MARK, pos, 0, 0); pos += 4; continue; }
      if (marker == 0xfffffffeu) emit(&w, RT_TAP_MESSAGE, pos, 0, RT_TAP_MSG_ERASED_GAP);
      pos += 4;
      const uint32_t length = marker & 0xffffffu;
      if (marker & 0x7f000000u) { st = RT_TAP_BAD_MARKER; snprintf(msg, sizeof msg, ".tap bad marker: %08lX", (unsigned long)marker); break; }
      if (length == 0) { st = RT_TAP_BAD_LENGTH; snprintf(msg, sizeof msg, ".tap bad record length: %08lX", (unsigned long)marker); break; }
      if (length >= RT_TEXT_MAXBLOCK) { st = RT_TAP_TOO_BIG; snprintf(msg, sizeof msg, ".tap data record too big: %d", (int)length); break; }
      if (nbytes - pos < length) { st = RT_TAP_EOF_TOO_SOON; snprintf(msg, sizeof msg, ".tap endfile too soon"); break; }
      emit(&w, RT_TAP_RECORD, pos, length, marker >> 31);
      pos += length;
      databytes += length;
      /* the trailing length: here, or 1 .. 4 bytes on */
      if (nbytes - pos < 4) {                                 /* (the reference says so in the text, then fails on the next byte it wants) */
         emit(&w, RT_TAP_MESSAGE, nbytes, 0, RT_TAP_MSG_NO_END);
         st = RT_TAP_EOF_TOO_SOON; snprintf(msg, sizeof msg, ".tap endfile too soon"); break; }
      int pad = 0;
      while ((le32(img + pos + pad) & 0xffffffu) != length) {
         if (pad == 4) { st = RT_TAP_NO_TRAILING_LENGTH; snprintf(msg, sizeof msg, "didn't find .tap trailing record length at file offset %lld", databytes); break; }
         if (nbytes - pos < (uint64_t)pad + 5) { st = RT_TAP_EOF_TOO_SOON; snprintf(msg, sizeof msg, ".tap endfile too soon"); break; }
         ++pad; ++databytes; }
      if (st != RT_TAP_OK) break;
      pos += 4 + (uint64_t)pad; }
   if (status) *status = st;
   if (err && errlen) snprintf(err, errlen, "%s", msg);
   return w.n; }

long long rt_tapread_write(const unsigned char *img, uint64_t nbytes, const char *base, const rt_text_options *o, const char *created,
                           int *status, char *err, size_t errlen) {
   int st = RT_TAP_OK;
   const int64_t n = rt_tap_items(img, nbytes, NULL, 0, &st, err, errlen);
   rt_tap_item *items = (rt_tap_item *)malloc((size_t)(n > 0 ? n : 1) * sizeof *items);
   if (!items) return -1;
   rt_tap_items(img, nbytes, items, n, &st, err, errlen);
   if (status) *status = st;
   struct rt_textfile *t = rt_text_new(base, o, 1, created);
   if (!t) { free(items); return -2; }
   if (rt_text_open_now(t)) { free(items); rt_text_close(t, 0); return -1; }      /* (the reference makes the file before it reads a marker) */
   for (int64_t i = 0; i < n; ++i) {
      const rt_tap_item *it = &items[i];
      if (it->kind == RT_TAP_RECORD) rt_text_record(t, img + it->offset, (int)it->length, it->flag ? 1 : 0, 0, NULL);
      else if (it->kind == RT_TAP_MARK) rt_text_tapemark(t, 0);
      else rt_text_message(t, rt_tap_messages[it->flag]); }
   free(items);
   return rt_text_close(t, st == RT_TAP_OK); }
