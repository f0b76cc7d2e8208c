/* rt_tapewrite.c — the tape writer's host side (rt_tapewrite.h): the encoders that turn a .tap image's items into flux transitions, and the reference
 * renderer.  The block formats are readtape_amd/synth.py's, restated: nrzi_words / nrzi_tapemark_words, pe_encode / pe_tapemark, gcr_encode; new here is the
 * GCR tape mark, the PE one at GCR density (300 ones on tracks 0 2 5 6 7 8, nothing on 1 3 4: what rt_decode_gcr.c's looks_like_tapemark counts).
 * A cell's word has track t in bit ntrks - 1 - t, as there; a slot's masks have track t in bit t. */
#include "rt_tapewrite.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rt_tapewrite_model.h"

enum { MODE_PE = 1, MODE_NRZI = 2, MODE_GCR = 4, MODE_WW = 8 };
enum { NRZI_SHORTEST = 10 };                 /* rt_decode_nrzi.c's SHORTEST_BLOCK: a block of so many cells or fewer that is no tape mark is dropped as noise */

static int refuse(int code, char *err, size_t errlen, const char *fmt, ...) {
   if (err && errlen) {
      va_list ap;
      va_start(ap, fmt);
      vsnprintf(err, errlen, fmt, ap);
      va_end(ap); }
   return code; }

static int finite_pos(double v) { return v > 0 && v < INFINITY; }
static int finite_nonneg(double v) { return v >= 0 && v < INFINITY; }

int rt_tapewrite_params(const rt_tapewrite_spec *s, int raw, rtfe_tape_params *out, char *err, size_t errlen) {
   if (!s || !out) return refuse(RT_TW_NULL, err, errlen, "rt_tapewrite_params: null argument");
   if (s->mode == MODE_WW)
      return refuse(RT_TW_BAD_SPEC, err, errlen, "Whirlwind tapes are not written: a Whirlwind pulse is two transitions 0.35 cell apart, which do not sit on the writer's half-cell grid");
   if (s->mode != MODE_PE && s->mode != MODE_NRZI && s->mode != MODE_GCR) return refuse(RT_TW_BAD_SPEC, err, errlen, "mode %d is not NRZI, PE or GCR", s->mode);
   if (raw ? (s->ntrks < 1 || s->ntrks > 19) : (s->mode == MODE_NRZI ? (s->ntrks != 7 && s->ntrks != 9) : s->ntrks != 9))
      return refuse(RT_TW_BAD_SPEC, err, errlen, "%d tracks: %s", s->ntrks, raw ? "1 to 19" : s->mode == MODE_NRZI ? "NRZI is written on 7 or 9" : "PE and GCR are written on 9");
   if (s->even && s->mode != MODE_NRZI) return refuse(RT_TW_BAD_SPEC, err, errlen, "even parity is NRZI's: PE and GCR are written with odd parity");
   if (!finite_pos(s->bpi) || !finite_pos(s->ips) || !finite_pos(s->tdelta_ns) || !finite_pos(s->maxvolts) || !finite_pos(s->pulse_w))
      return refuse(RT_TW_BAD_SPEC, err, errlen, "bpi %g, ips %g, tdelta %g ns, maxvolts %g, pulse width %g: each must be above 0", s->bpi, s->ips, s->tdelta_ns, s->maxvolts, s->pulse_w);
   if (!finite_nonneg(s->noise_mv) || !finite_nonneg(s->jitter) || s->gap_samples < 0 || !(fabs(s->amplitude) < INFINITY) || !(fabs(s->amp_slope) < INFINITY))
      return refuse(RT_TW_BAD_SPEC, err, errlen, "noise %g mV, jitter %g cells, gap %lld samples, amplitude %g, slope %g", s->noise_mv, s->jitter, (long long)s->gap_samples, s->amplitude, s->amp_slope);
   memset(out, 0, sizeof *out);
   out->ntrks = s->ntrks;
   out->pitch_shift = s->mode == MODE_PE;
   out->spb = 1.0 / (s->bpi * s->ips * s->tdelta_ns * 1e-9);                   /* synth.TapeSpec.samples_per_bit */
   out->w = s->pulse_w * out->spb;
   const double k = ceil(16.0 * out->w);                                        /* synth._render_pulses */
   if (!finite_pos(out->spb) || !finite_pos(out->w) || !(k < 1e9)) return refuse(RT_TW_BAD_SPEC, err, errlen, "%g samples a cell with a pulse %g samples wide", out->spb, out->w);
   out->K = (int32_t)k;
   out->edge = 1.0 / (1.0 + (k / out->w) * (k / out->w));
   out->maxvolts = s->maxvolts; out->noise_mv = s->noise_mv; out->jitter = s->jitter;
   const uint64_t base = rt_tw_mix(s->seed + RT_TW_GOLDEN);
   for (int t = 0; t < s->ntrks; ++t) {
      if (!(fabs(s->skew_cells[t]) < INFINITY)) return refuse(RT_TW_BAD_SPEC, err, errlen, "track %d: a skew of %g cells", t, s->skew_cells[t]);
      out->amp[t] = s->amplitude * (1.0 + s->amp_slope * t);
      out->skew[t] = s->skew_cells[t];
      out->nkey[t] = rt_tw_mix(base ^ (uint64_t)(0x4E00 + t));
      out->jkey[t] = rt_tw_mix(base ^ (uint64_t)(0x4A00 + t)); }
   return RT_TW_OK; }

/* ---- a plan under construction ---- */
struct build {
   rt_tapewrite_plan *plan;
   int64_t slot_cap, block_cap, row;
   uint32_t *cells; int64_t cell_cap, ncells;      /* the block being encoded: a word a cell */
};

static int grow(void **p, int64_t *cap, int64_t need, size_t each) {
   if (need <= *cap) return 0;
   int64_t n = *cap ? *cap : 1024;
   while (n < need) n *= 2;
   void *q = realloc(*p, (size_t)n * each);
   if (!q) return -1;
   *p = q; *cap = n;
   return 0; }

static int cell(struct build *b, uint32_t word) {
   if (grow((void **)&b->cells, &b->cell_cap, b->ncells + 1, sizeof *b->cells)) return -1;
   b->cells[b->ncells++] = word;
   return 0; }

static uint32_t track_mask(uint32_t word, int ntrks) {
   uint32_t m = 0;
   for (int t = 0; t < ntrks; ++t) m |= ((word >> (ntrks - 1 - t)) & 1u) << t;
   return m; }

/* a block of nslots slots (already in the plan's stream) and ncells cells takes its rows behind `gap` rows of gap */
static int place(struct build *b, int64_t gap, int64_t first_slot, int64_t nslots, double ncells) {
   rt_tapewrite_plan *P = b->plan;
   if (grow((void **)&P->blocks, &b->block_cap, P->nblocks + 1, sizeof *P->blocks)) return -1;
   const double rows = ceil((ncells + 2 * RT_TW_LEAD) * P->params.spb);         /* synth._render_block */
   if (!(rows >= 1 && rows < 9e15)) return -2;
   b->row += gap;
   const rtfe_tape_block B = { b->row, (int64_t)rows, first_slot, nslots };
   P->blocks[P->nblocks++] = B;
   b->row += (int64_t)rows;
   return 0; }

/* the cells gathered in b->cells -> slots.  NRZI and GCR: a one is a transition at its cell's centre, a slot a cell.  PE (synth._pe_track_transitions): on
 * the tracks of `active` every cell has a transition at its centre - slot 2k, up for a one and down for a zero - and one at the boundary in front of it -
 * slot 2k - 1 - where it repeats its predecessor's bit.  A track's pulses alternate; the first is negative for the tracks of first_neg. */
static int emit_block(struct build *b, int pe, uint32_t active, uint32_t first_neg, int64_t gap) {
   rt_tapewrite_plan *P = b->plan;
   const int ntrks = P->params.ntrks;
   const int64_t n = b->ncells, nslots = pe ? (n > 0 ? 2 * n - 1 : 0) : n, first = P->nslots;
   if (nslots > 0x7fffffffll) return -2;
   if (grow((void **)&P->slots, &b->slot_cap, P->nslots + nslots, sizeof *P->slots)) return -1;
   uint32_t state = first_neg, prev = 0;
   for (int64_t k = 0; k < n; ++k) {
      const uint32_t m = track_mask(b->cells[k], ntrks);
      if (pe && k > 0) {
         const rtfe_tape_slot s = { active & ~(m ^ prev), state & active & ~(m ^ prev) };
         P->slots[P->nslots++] = s;
         state ^= s.flux; }
      const rtfe_tape_slot s = { pe ? active : m, state & (pe ? active : m) };
      P->slots[P->nslots++] = s;
      state ^= s.flux;
      prev = m; }
   const int rc = place(b, gap, first, nslots, (double)n);
   b->ncells = 0;
   return rc; }

static int parity8(unsigned v) { v ^= v >> 4; v ^= v >> 2; v ^= v >> 1; return (int)(v & 1u); }

/* synth.nrzi_words: the data words (data << 1 | P), then 0 0 0 CRC 0 0 0 LRC on nine tracks, 0 0 0 LRC 0 0 0 0 on seven */
static int nrzi_record(struct build *b, const unsigned char *d, uint32_t n, int ntrks, int even, int64_t item, char *err, size_t errlen) {
   const unsigned top = (1u << (ntrks - 1)) - 1;
   uint32_t crc = 0, lrc = 0;
   if (n + 8 <= NRZI_SHORTEST)
      return refuse(RT_TW_BAD_ITEM, err, errlen, "item %lld: an NRZI record of %u bytes is a block of %u cells, and one of %d or fewer is noise to every NRZI decoder: 3 bytes at the least", (long long)item, n, n + 8, NRZI_SHORTEST);
   for (uint32_t i = 0; i < n; ++i) {
      if (d[i] > top) return refuse(RT_TW_BAD_ITEM, err, errlen, "item %lld: byte %u of the record is 0x%02X, which %d data tracks cannot carry", (long long)item, i, d[i], ntrks - 1);
      const uint32_t w = (uint32_t)d[i] << 1 | (uint32_t)(parity8(d[i]) ^ (even ? 0 : 1));
      if (w == 0) return refuse(RT_TW_BAD_ITEM, err, errlen, "item %lld: byte %u of the record is zero, under even parity a cell without any flux, which no NRZI reader can count", (long long)item, i);
      if (cell(b, w)) return RT_TW_NO_MEMORY;
      lrc ^= w;
      crc ^= w;
      if (crc & 2) crc ^= 0xF0;
      const uint32_t lsb = crc & 1;
      crc >>= 1;
      if (lsb) crc |= 0x100; }
   crc ^= 0x1AF;
   const uint32_t tail9[8] = { 0, 0, 0, crc, 0, 0, 0, lrc ^ crc }, tail7[8] = { 0, 0, 0, lrc, 0, 0, 0, 0 };
   for (int i = 0; i < 8; ++i) if (cell(b, ntrks == 9 ? tail9[i] : tail7[i])) return RT_TW_NO_MEMORY;
   return 0; }

static int nrzi_mark(struct build *b, int ntrks) {
   static const uint32_t m9[9] = { 0x26, 0, 0, 0, 0, 0, 0, 0, 0x26 }, m7[5] = { 0x1E, 0, 0, 0, 0x1E };
   for (int i = 0; i < (ntrks == 9 ? 9 : 5); ++i) if (cell(b, ntrks == 9 ? m9[i] : m7[i])) return RT_TW_NO_MEMORY;
   return 0; }

/* synth.pe_encode: 40 zeros, a one, the data, a one, 40 zeros on every track */
static int pe_record(struct build *b, const unsigned char *d, uint32_t n) {
   for (int i = 0; i < 40; ++i) if (cell(b, 0)) return RT_TW_NO_MEMORY;
   if (cell(b, 0x1FF)) return RT_TW_NO_MEMORY;
   for (uint32_t i = 0; i < n; ++i) if (cell(b, (uint32_t)d[i] << 1 | (uint32_t)(parity8(d[i]) ^ 1))) return RT_TW_NO_MEMORY;
   if (cell(b, 0x1FF)) return RT_TW_NO_MEMORY;
   for (int i = 0; i < 40; ++i) if (cell(b, 0)) return RT_TW_NO_MEMORY;
   return 0; }

/* ---- GCR (synth.gcr_encode) ---- */
static const uint32_t GCR_4TO5[16] = { 0x19, 0x1B, 0x12, 0x13, 0x1D, 0x15, 0x16, 0x17, 0x1A, 0x09, 0x0A, 0x0B, 0x1E, 0x0D, 0x0E, 0x0F };
static const uint64_t GCR_ECC_ROWS[8] = { 0x0f6a71994c5230ull, 0x70110840108004ull, 0x5a701108401080ull, 0x372be95d5a7011ull,
                                          0xe95d5a70110840ull, 0x4c523001884412ull, 0x2be95d5a701108ull, 0x5d5a7011084010ull };

static unsigned gcr_ecc(const unsigned char *seven) {
   uint64_t word = 0;
   for (int i = 0; i < 7; ++i) word = word << 8 | seven[i];
   unsigned e = 0;
   for (int i = 0; i < 8; ++i) e |= (unsigned)__builtin_parityll(word & GCR_ECC_ROWS[i]) << i;
   return e; }

static int gcr_ctl(struct build *b, unsigned code) {
   for (int k = 0; k < 5; ++k) if (cell(b, (code >> (4 - k)) & 1u ? 0x1FF : 0)) return RT_TW_NO_MEMORY;
   return 0; }

/* seven characters and their check character -> ten cells: two 5-bit storage groups a track */
static int gcr_group(struct build *b, const unsigned char *seven) {
   uint32_t words[8], cells[10] = { 0 };
   for (int i = 0; i < 8; ++i) {
      const unsigned c = i < 7 ? seven[i] : gcr_ecc(seven);
      words[i] = c << 1 | (uint32_t)(parity8(c) ^ 1); }
   for (int trk = 0; trk < 9; ++trk)
      for (int half = 0; half < 2; ++half) {
         unsigned nib = 0;
         for (int i = 0; i < 4; ++i) nib = nib << 1 | ((words[4 * half + i] >> (8 - trk)) & 1u);
         const uint32_t code = GCR_4TO5[nib];
         for (int k = 0; k < 5; ++k) if ((code >> (4 - k)) & 1u) cells[5 * half + k] |= 1u << (8 - trk); }
   for (int k = 0; k < 10; ++k) if (cell(b, cells[k])) return RT_TW_NO_MEMORY;
   return 0; }

static int gcr_record(struct build *b, const unsigned char *d, uint32_t n) {
   int rc = gcr_ctl(b, 0x15) || gcr_ctl(b, 0x0F);
   for (int i = 0; i < 14 && !rc; ++i) rc = gcr_ctl(b, 0x1F);
   if (!rc) rc = gcr_ctl(b, 0x07);                                              /* MARK1: data starts */
   const uint32_t nfull = n / 7, left = n % 7;
   for (uint32_t g = 0; g < nfull && !rc; ++g) rc = gcr_group(b, d + 7 * g);
   if (!rc) rc = gcr_ctl(b, 0x1F);                                              /* end of the data groups */
   unsigned char resid[7] = { 0 }, crc[7] = { 0 };                              /* H H H H H H N; B C C C C C X, X's top three bits = the residual count */
   memcpy(resid, d + 7 * nfull, left);
   crc[6] = (unsigned char)(left << 5);
   if (!rc) rc = gcr_group(b, resid) || gcr_group(b, crc);
   if (!rc) rc = gcr_ctl(b, 0x1C);                                              /* MARK2 */
   for (int i = 0; i < 14 && !rc; ++i) rc = gcr_ctl(b, 0x1F);
   if (!rc) rc = gcr_ctl(b, 0x1E) || gcr_ctl(b, 0x15);
   return rc ? RT_TW_NO_MEMORY : 0; }

enum { MARK_TRACKS = 0x1FF & ~(1 << 1 | 1 << 3 | 1 << 4) };                      /* a PE / GCR tape mark: tracks 0 2 5 6 7 8 (slot masks: track t in bit t) */

static struct build *build_new(const rt_tapewrite_spec *s, int raw, int *rc, char *err, size_t errlen) {
   rtfe_tape_params p;
   *rc = rt_tapewrite_params(s, raw, &p, err, errlen);
   if (*rc) return NULL;
   struct build *b = (struct build *)calloc(1, sizeof *b);
   if (b) b->plan = (rt_tapewrite_plan *)calloc(1, sizeof *b->plan);
   if (!b || !b->plan) { free(b); *rc = refuse(RT_TW_NO_MEMORY, err, errlen, "out of memory"); return NULL; }
   b->plan->params = p;
   return b; }

static int build_end(struct build *b, int rc, int64_t tail_gap, rt_tapewrite_plan **plan, char *err, size_t errlen) {
   rt_tapewrite_plan *P = b->plan;
   free(b->cells);
   P->total_rows = b->row + tail_gap;
   free(b);
   if (rc == -1 || rc == RT_TW_NO_MEMORY) rc = refuse(RT_TW_NO_MEMORY, err, errlen, "out of memory");
   else if (rc == -2) rc = refuse(RT_TW_BAD_ITEM, err, errlen, "a block of more than 2^31 - 1 slots, or of more rows than a tape has");
   if (rc) { rt_tapewrite_free(P); return rc; }
   *plan = P;
   return RT_TW_OK; }

void rt_tapewrite_free(rt_tapewrite_plan *plan) {
   if (!plan) return;
   free(plan->slots); free(plan->blocks); free(plan); }

int rt_tapewrite_encode(const unsigned char *img, uint64_t nbytes, const rt_tap_item *items, int64_t nitems, const rt_tapewrite_spec *s,
                        rt_tapewrite_plan **plan, char *err, size_t errlen) {
   if (!s || !plan || nitems < 0 || (nitems > 0 && !items) || (nbytes > 0 && !img)) return refuse(RT_TW_NULL, err, errlen, "rt_tapewrite_encode: null argument");
   *plan = NULL;
   int rc = 0;
   struct build *b = build_new(s, 0, &rc, err, errlen);
   if (!b) return rc;
   const int ntrks = s->ntrks, pe = s->mode == MODE_PE;
   for (int64_t i = 0; i < nitems && !rc; ++i) {
      const rt_tap_item *it = &items[i];
      if (it->kind == RT_TAP_MESSAGE) continue;
      uint32_t active = (1u << ntrks) - 1, first_neg = 0;
      if (it->kind == RT_TAP_MARK) {
         if (s->mode == MODE_NRZI) rc = nrzi_mark(b, ntrks);
         else {                                                                 /* synth.pe_tapemark: 45 zero cells (90 flux changes); GCR: 300 ones */
            active = MARK_TRACKS;
            for (int k = 0; k < (pe ? 45 : 300) && !rc; ++k) rc = cell(b, pe ? 0 : 0x1FF & ~(1u << 7 | 1u << 5 | 1u << 4)) ? RT_TW_NO_MEMORY : 0; } }
      else if (it->kind == RT_TAP_RECORD) {
         if (it->length < 1 || it->offset > nbytes || nbytes - it->offset < it->length) {
            rc = refuse(RT_TW_BAD_ITEM, err, errlen, "item %lld: a record of %u bytes at offset %llu lies outside the image of %llu bytes", (long long)i, it->length, (unsigned long long)it->offset, (unsigned long long)nbytes);
            break; }
         const unsigned char *d = img + it->offset;
         rc = s->mode == MODE_NRZI ? nrzi_record(b, d, it->length, ntrks, s->even, i, err, errlen) : pe ? pe_record(b, d, it->length) : gcr_record(b, d, it->length);
         if (rc == RT_TW_BAD_ITEM) break; }
      else { rc = refuse(RT_TW_BAD_ITEM, err, errlen, "item %lld is of kind %d: neither a record nor a tape mark", (long long)i, (int)it->kind); break; }
      if (pe) first_neg = active & ~track_mask(b->ncells ? b->cells[0] : 0, ntrks);     /* a PE track's first pulse is negative where its first bit is zero */
      if (!rc) rc = emit_block(b, pe, active, first_neg, s->gap_samples); }
   if (rc == RT_TW_BAD_ITEM) { free(b->cells); rt_tapewrite_free(b->plan); free(b); return rc; }
   return build_end(b, rc, s->gap_samples, plan, err, errlen); }

int rt_tapewrite_raw(const rtfe_tape_slot *slots, const int64_t *block_slots, const double *block_cells, const int64_t *gap_before, int64_t nblocks,
                     const rt_tapewrite_spec *s, rt_tapewrite_plan **plan, char *err, size_t errlen) {
   if (!s || !plan || nblocks < 0 || (nblocks > 0 && (!block_slots || !block_cells))) return refuse(RT_TW_NULL, err, errlen, "rt_tapewrite_raw: null argument");
   *plan = NULL;
   int rc = 0;
   struct build *b = build_new(s, 1, &rc, err, errlen);
   if (!b) return rc;
   rt_tapewrite_plan *P = b->plan;
   const uint32_t all = (1u << s->ntrks) - 1;
   int64_t at = 0;
   for (int64_t k = 0; k < nblocks && !rc; ++k) {
      const int64_t n = block_slots[k];
      if (n < 0 || n > 0x7fffffffll || (n > 0 && !slots) || !(block_cells[k] >= 0 && block_cells[k] < 9e15) || (gap_before && gap_before[k] < 0)) {
         rc = refuse(RT_TW_BAD_ITEM, err, errlen, "block %lld: %lld slots, %g cells, a gap of %lld rows", (long long)k, (long long)n, block_cells[k], (long long)(gap_before ? gap_before[k] : 0));
         break; }
      if (grow((void **)&P->slots, &b->slot_cap, P->nslots + n, sizeof *P->slots)) { rc = -1; break; }
      for (int64_t i = 0; i < n; ++i) {
         const rtfe_tape_slot sl = slots[at + i];
         if ((sl.flux & ~all) || (sl.neg & ~sl.flux)) {
            rc = refuse(RT_TW_BAD_ITEM, err, errlen, "block %lld, slot %lld: masks %08X / %08X on %d tracks", (long long)k, (long long)i, sl.flux, sl.neg, s->ntrks);
            break; }
         P->slots[P->nslots + i] = sl; }
      if (rc) break;
      P->nslots += n;
      rc = place(b, gap_before ? gap_before[k] : s->gap_samples, P->nslots - n, n, block_cells[k]);
      at += n; }
   if (rc == RT_TW_BAD_ITEM) { free(b->cells); rt_tapewrite_free(b->plan); free(b); return rc; }
   return build_end(b, rc, s->gap_samples, plan, err, errlen); }

int rt_tapewrite_render(const rtfe_tape_slot *slots, int64_t nslots, const rtfe_tape_block *blocks, int64_t nblocks, const rtfe_tape_params *p,
                        int64_t first_row, int64_t nrows, int16_t *rows, char *err, size_t errlen) {
   if (!p || (nrows > 0 && !rows) || (nslots > 0 && !slots) || (nblocks > 0 && !blocks)) return refuse(RT_TW_NULL, err, errlen, "rt_tapewrite_render: null argument");
   if (p->ntrks < 1 || p->ntrks > 19 || nslots < 0 || nblocks < 0 || first_row < 0 || nrows < 0 || first_row > INT64_MAX - nrows || p->K < 0)
      return refuse(RT_TW_BAD_SPEC, err, errlen, "rt_tapewrite_render: %d tracks, %lld slots, %lld blocks, rows %lld + %lld", p->ntrks, (long long)nslots, (long long)nblocks, (long long)first_row, (long long)nrows);
   int64_t row = 0;
   for (int64_t b = 0; b < nblocks; ++b) {
      const rtfe_tape_block *B = &blocks[b];
      if (B->first_row < row || B->rows < 1 || B->rows > INT64_MAX - B->first_row || B->first_slot < 0 || B->nslots < 0 || B->first_slot > nslots || B->nslots > nslots - B->first_slot)
         return refuse(RT_TW_BAD_TABLE, err, errlen, "rt_tapewrite_render: block %lld of the table is out of order or out of range", (long long)b);
      row = B->first_row + B->rows; }
   if (nrows == 0) return RT_TW_OK;
   const int nt = p->ntrks;
   const int64_t w1 = first_row + nrows;
   double *acc = (double *)calloc((size_t)nrows * (size_t)nt, sizeof *acc);     /* volts, before the noise: every sample starts from 0.0 */
   if (!acc) return refuse(RT_TW_NO_MEMORY, err, errlen, "rt_tapewrite_render: out of memory for a window of %lld rows", (long long)nrows);
   for (int64_t b = 0; b < nblocks; ++b) {
      const rtfe_tape_block *B = &blocks[b];
      if (B->first_row >= w1) break;
      if (B->first_row + B->rows <= first_row) continue;
      const int64_t q0 = (B->first_row > first_row ? B->first_row : first_row) - B->first_row;      /* the block's rows [q0, q1) lie in the window */
      const int64_t q1 = (B->first_row + B->rows < w1 ? B->first_row + B->rows : w1) - B->first_row;
      for (int t = 0; t < nt; ++t)
         for (int64_t s = 0; s < B->nslots; ++s) {                              /* pulse after pulse, in the order they were written */
            const rtfe_tape_slot sl = slots[B->first_slot + s];
            if (!((sl.flux >> t) & 1u)) continue;
            const double c = rt_tw_centre(p->spb, p->pitch_shift, p->skew[t], p->jitter, p->jkey[t], s, B->first_slot + s);
            if (!(c > -4e18 && c < 4e18)) continue;                             /* (no such centre reaches a row) */
            const int64_t base = (int64_t)rint(c);
            const int64_t r0 = base - p->K > q0 ? base - p->K : q0, r1 = base + p->K < q1 - 1 ? base + p->K : q1 - 1;
            const double a = ((sl.neg >> t) & 1u) ? -p->amp[t] : p->amp[t];
            for (int64_t r = r0; r <= r1; ++r) acc[(size_t)(B->first_row + r - first_row) * nt + t] += rt_tw_pulse(a, r, c, p->w, p->edge); } }
   for (int64_t i = 0; i < nrows; ++i)
      for (int t = 0; t < nt; ++t)
         rows[(size_t)i * nt + t] = rt_tw_quantise(acc[(size_t)i * nt + t] + rt_tw_noise(p->noise_mv, p->nkey[t], first_row + i), p->maxvolts);
   free(acc);
   return RT_TW_OK; }
