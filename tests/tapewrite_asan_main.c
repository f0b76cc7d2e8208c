/* tapewrite_asan_main.c — the tape writer's encoder and host renderer (csrc/host/rt_tapewrite.c) behind the .tap reader (rt_tapread.c) in a program of their
 * own, for a sanitizer run on the CPU - the lengths in a .tap image are untrusted input:
 *
 *   gcc -std=gnu99 -O1 -g -fsanitize=address,undefined -static-libasan -fno-sanitize-recover=all -ffp-contract=off -D_DEFAULT_SOURCE -Ireadtape_amd/csrc/host -Iinclude \
 *       -o tapewrite_asan tests/tapewrite_asan_main.c readtape_amd/csrc/host/rt_tapewrite.c readtape_amd/csrc/host/rt_tapread.c readtape_amd/csrc/host/rt_textfile.c -lm
 *   ./tapewrite_asan
 *
 * It builds an image of records and tape marks, and runs reader, encoder and renderer over it whole, over every truncation of it (each in a heap block of
 * exactly its size, so that a read behind the end is seen), over images whose length fields are larger than the image, over an empty one, and over item
 * tables that lie about the image; then the raw encoder and the renderer's own refusals.  Prints "ok". */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rt_tapewrite.h"
#include "rt_textfile.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static size_t put32(unsigned char *p, uint32_t v) { p[0] = (unsigned char)v; p[1] = (unsigned char)(v >> 8); p[2] = (unsigned char)(v >> 16); p[3] = (unsigned char)(v >> 24); return 4; }
static size_t put_record(unsigned char *p, uint32_t n, uint32_t marker) {
   size_t at = put32(p, marker);
   for (uint32_t i = 0; i < n; ++i) p[at++] = (unsigned char)(1 + (i * 7 + n) % 63);      /* 1 .. 63: fits seven tracks, no zero byte */
   if (n & 1) p[at++] = 0;
   return at + put32(p + at, marker); }

static rt_tapewrite_spec spec_of(int mode, int ntrks) {
   rt_tapewrite_spec s;
   memset(&s, 0, sizeof s);
   s.mode = mode; s.ntrks = ntrks;
   s.bpi = mode == 4 ? 9042 : mode == 1 ? 1600 : 800; s.ips = 50; s.tdelta_ns = mode == 4 ? 160 : mode == 1 ? 640 : 1280;
   s.maxvolts = 4.4; s.amplitude = 2.5; s.amp_slope = 0.03; s.pulse_w = mode == 1 ? 0.13 : 0.22; s.noise_mv = 10; s.jitter = 0.02;
   for (int t = 0; t < ntrks; ++t) s.skew_cells[t] = 0.05 * (t % 3);
   s.gap_samples = 37; s.seed = 9;
   return s; }

/* reader -> encoder -> renderer (whole, and three windows) over nbytes of img copied into a block of their own -> the encoder's code */
static int through(const unsigned char *img, size_t nbytes, const rt_tapewrite_spec *s, long *rendered) {
   unsigned char *own = (unsigned char *)malloc(nbytes ? nbytes : 1);
   CHECK(own);
   memcpy(own, img, nbytes);
   int st = 0;
   char err[200];
   const int64_t n = rt_tap_items(own, nbytes, NULL, 0, &st, err, sizeof err);
   rt_tap_item *items = (rt_tap_item *)malloc((size_t)(n > 0 ? n : 1) * sizeof *items);
   CHECK(items && rt_tap_items(own, nbytes, items, n, &st, err, sizeof err) == n);
   rt_tapewrite_plan *plan = NULL;
   const int rc = rt_tapewrite_encode(own, nbytes, items, n, s, &plan, err, sizeof err);
   if (rc == RT_TW_OK) {
      CHECK(plan && plan->total_rows >= s->gap_samples);
      const int64_t total = plan->total_rows, cuts[4][2] = { { 0, total }, { 0, total / 3 }, { total / 3, total - total / 3 }, { total - 1, 1 } };
      for (int c = 0; c < 4; ++c) {
         int16_t *rows = (int16_t *)malloc((size_t)(cuts[c][1] * s->ntrks + 1) * sizeof *rows);
         CHECK(rows);
         CHECK(rt_tapewrite_render(plan->slots, plan->nslots, plan->blocks, plan->nblocks, &plan->params, cuts[c][0], cuts[c][1], rows, err, sizeof err) == RT_TW_OK);
         free(rows);
         ++*rendered; }
      rt_tapewrite_free(plan); }
   else CHECK(plan == NULL && err[0]);
   free(items); free(own);
   return rc; }

int main(void) {
   static unsigned char img[40000];
   size_t n = 0;
   n += put32(img + n, 0);                                                    /* a tape mark first */
   n += put_record(img + n, 12, 12);
   n += put_record(img + n, 13, 13 | 0x80000000u);                            /* flagged bad: written as data */
   n += put32(img + n, 0); n += put32(img + n, 0);
   n += put_record(img + n, 4099, 4099);
   n += put_record(img + n, 3, 3);
   n += put32(img + n, 0);
   n += put32(img + n, 0xffffffffu);
   long rendered = 0;
   const int modes[4][2] = { { 2, 9 }, { 2, 7 }, { 1, 9 }, { 4, 9 } };
   for (int m = 0; m < 4; ++m) {
      const rt_tapewrite_spec s = spec_of(modes[m][0], modes[m][1]);
      CHECK(through(img, n, &s, &rendered) == RT_TW_OK);
      for (size_t cut = 0; cut < n; cut += (cut < 80 || cut + 80 > n ? 1 : 397)) through(img, cut, &s, &rendered);      /* truncated, the empty image included */
      /* a length field larger than the image, at the first record's marker, at its trailer, at both */
      static unsigned char bad[40000];
      const uint32_t big[4] = { 0x00ffffffu, 0x0001ffffu, 40000u, 13u };
      for (int k = 0; k < 4; ++k) for (int where = 1; where <= 3; ++where) {
         memcpy(bad, img, n);
         if (where & 1) put32(bad + 4, big[k]);
         if (where & 2) put32(bad + 4 + 4 + 12, big[k]);
         through(bad, n, &s, &rendered); }
      /* an item table that lies: a record that ends behind the image, one that starts there, one of no length, one of no known kind */
      const rt_tap_item lies[4] = { { n - 4, 8, RT_TAP_RECORD, 0 }, { n + 1, 4, RT_TAP_RECORD, 0 }, { 8, 0, RT_TAP_RECORD, 0 }, { 8, 12, 7, 0 } };
      for (int k = 0; k < 4; ++k) {
         rt_tapewrite_plan *plan = NULL;
         char err[200] = "";
         CHECK(rt_tapewrite_encode(img, n, &lies[k], 1, &s, &plan, err, sizeof err) == RT_TW_BAD_ITEM && !plan && err[0]); } }
   /* what the formats cannot carry */
   rt_tapewrite_spec s7 = spec_of(2, 7), se = spec_of(2, 9), sw = spec_of(8, 6), sp = spec_of(1, 7);
   se.even = 1;
   static unsigned char one[64];
   size_t m = put32(one, 4);
   one[4] = 1; one[5] = 0x40; one[6] = 0; one[7] = 2;
   m = 8 + put32(one + 8, 4);
   m += put32(one + m, 0xffffffffu);
   CHECK(through(one, m, &s7, &rendered) == RT_TW_BAD_ITEM);                  /* 0x40 on six data tracks */
   CHECK(through(one, m, &se, &rendered) == RT_TW_BAD_ITEM);                  /* a zero byte under even parity */
   CHECK(through(one, m, &sw, &rendered) == RT_TW_BAD_SPEC && through(one, m, &sp, &rendered) == RT_TW_BAD_SPEC);
   put32(one, 2); put32(one + 6, 2); put32(one + 10, 0xffffffffu);
   se.even = 0;
   CHECK(through(one, 14, &se, &rendered) == RT_TW_BAD_ITEM);                 /* two bytes: noise to an NRZI decoder */
   /* raw masks, nineteen tracks, and the renderer's refusals */
   rt_tapewrite_spec s19 = spec_of(2, 19);
   rtfe_tape_slot slots[50];
   for (int i = 0; i < 50; ++i) { slots[i].flux = (uint32_t)(i * 2654435761u) & 0x7ffffu; slots[i].neg = slots[i].flux & (uint32_t)(i * 40503u); }
   const int64_t counts[3] = { 20, 0, 30 }, gaps[3] = { 5, 0, 700 };
   const double cells[3] = { 20, 0, 31.5 };
   rt_tapewrite_plan *plan = NULL;
   char err[200];
   CHECK(rt_tapewrite_raw(slots, counts, cells, gaps, 3, &s19, &plan, err, sizeof err) == RT_TW_OK && plan->nblocks == 3 && plan->nslots == 50);
   int16_t *rows = (int16_t *)malloc((size_t)plan->total_rows * 19 * sizeof *rows);
   CHECK(rows && rt_tapewrite_render(plan->slots, plan->nslots, plan->blocks, plan->nblocks, &plan->params, 0, plan->total_rows, rows, err, sizeof err) == RT_TW_OK);
   rtfe_tape_block swapped[3] = { plan->blocks[2], plan->blocks[1], plan->blocks[0] };
   CHECK(rt_tapewrite_render(plan->slots, plan->nslots, swapped, 3, &plan->params, 0, 10, rows, err, sizeof err) == RT_TW_BAD_TABLE);
   CHECK(rt_tapewrite_render(plan->slots, 49, plan->blocks, 3, &plan->params, 0, 10, rows, err, sizeof err) == RT_TW_BAD_TABLE);
   CHECK(rt_tapewrite_render(plan->slots, plan->nslots, plan->blocks, 3, &plan->params, -1, 10, rows, err, sizeof err) == RT_TW_BAD_SPEC);
   slots[7].flux = 1u << 19;
   rt_tapewrite_plan *none = NULL;
   CHECK(rt_tapewrite_raw(slots, counts, cells, gaps, 3, &s19, &none, err, sizeof err) == RT_TW_BAD_ITEM && !none);
   free(rows);
   rt_tapewrite_free(plan);
   printf("ok: %ld windows rendered\n", rendered);
   return 0; }
