/* rt_tapewrite.h — the tape writer's host side: a SIMH .tap image -> flux transitions (a slot stream and a block table), and the reference renderer that
 * turns them into the int16 rows a head would have read.  The device renderer is rtfe_tape_render (include/rt_frontend.h), where the model is stated; the
 * expressions both share are rt_tapewrite_model.h.  The formats are the ones readtape_amd/synth.py writes for the tests, restated from it. */
#ifndef RT_TAPEWRITE_H
#define RT_TAPEWRITE_H
#include <stddef.h>
#include <stdint.h>

#include "rt_frontend.h"
#include "rt_text_tables.h"

/* the physical description of a tape to write (readtape_amd/tapewrite.py: WriteSpec) */
typedef struct rt_tapewrite_spec {
   int32_t mode, ntrks, even, reserved;      /* mode: the TBIN header's number (PE 1, NRZI 2, GCR 4); even: NRZI's even parity */
   double bpi, ips, tdelta_ns, maxvolts, amplitude, amp_slope, pulse_w, noise_mv, jitter;
   double skew_cells[19];
   int64_t gap_samples;                      /* rows of gap in front of, between and behind the blocks */
   uint64_t seed;
} rt_tapewrite_spec;

/* what the encoders return (rt_tapewrite_free) */
typedef struct rt_tapewrite_plan {
   rtfe_tape_slot *slots; int64_t nslots;
   rtfe_tape_block *blocks; int64_t nblocks;      /* sorted by first_row */
   int64_t total_rows;
   rtfe_tape_params params;
} rt_tapewrite_plan;

enum { RT_TW_OK = 0, RT_TW_NULL = -1, RT_TW_BAD_SPEC = -2, RT_TW_BAD_ITEM = -3, RT_TW_NO_MEMORY = -4, RT_TW_BAD_TABLE = -5 };

/* The renderers' parameters of a description: spb = 1 / (bpi * ips * tdelta_ns * 1e-9), w = pulse_w * spb, K = ceil(16 w), edge, the tracks' amplitudes and
 * the generator's keys.  raw != 0 admits 1 .. 19 tracks (rt_tapewrite_raw); otherwise NRZI wants 7 or 9, PE and GCR 9, and `even` NRZI.  Whirlwind (mode 8)
 * is refused: its pulse pairs lie 0.35 cell apart and do not sit on the half-cell grid of the slots.  0, or RT_TW_BAD_SPEC with err saying why. */
int rt_tapewrite_params(const rt_tapewrite_spec *s, int raw, rtfe_tape_params *out, char *err, size_t errlen);

/* The items of an image (rt_tap_items' table: records, tape marks; its messages are no part of the tape and are passed over; a record whose marker has the
 * error bit is written as data) -> a plan.  An item the format cannot carry - a byte above 63 on seven tracks, a zero byte under even parity (a cell with no
 * flux at all, which no NRZI reader can count), an NRZI record of one or two bytes (with its eight trailer cells a block of ten cells or fewer, which every NRZI
 * decoder, the reference's included, drops as noise), a record outside the image, an item of no known kind - is refused, RT_TW_BAD_ITEM, err naming it. */
int rt_tapewrite_encode(const unsigned char *img, uint64_t nbytes, const rt_tap_item *items, int64_t nitems, const rt_tapewrite_spec *s,
                        rt_tapewrite_plan **plan, char *err, size_t errlen);

/* Slot masks given directly, 1 .. 19 tracks: block b has block_slots[b] slots (consecutive in `slots`) and block_cells[b] cells - it takes
 * ceil((cells + 16) * spb) rows - behind gap_before[b] rows of gap (NULL: s->gap_samples each); s->gap_samples rows follow the last.  The slots' pitch is
 * the mode's (PE: half a cell).  A flux or neg bit at or above ntrks, a neg bit without its flux bit: RT_TW_BAD_ITEM. */
int rt_tapewrite_raw(const rtfe_tape_slot *slots, const int64_t *block_slots, const double *block_cells, const int64_t *gap_before, int64_t nblocks,
                     const rt_tapewrite_spec *s, rt_tapewrite_plan **plan, char *err, size_t errlen);
void rt_tapewrite_free(rt_tapewrite_plan *plan);

/* The model in plain C: rows [first_row, first_row + nrows) of the tape into rows[0 .. nrows * ntrks).  What rtfe_tape_render is held against, and the host
 * path of the writer.  RT_TW_BAD_TABLE: the block table is out of order or names slots outside the stream (rtfe_tape_render's -61). */
int rt_tapewrite_render(const rtfe_tape_slot *slots, int64_t nslots, const rtfe_tape_block *blocks, int64_t nblocks, const rtfe_tape_params *p,
                        int64_t first_row, int64_t nrows, int16_t *rows, char *err, size_t errlen);
#endif
